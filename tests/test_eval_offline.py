"""CPU: the offline evaluator's host side (rdmnet_amd/eval.py, evaluation.Summary.commit_record, the C-ABI bindings) and the
float64 restatement the GPU tests lean on, against what the reference's own evaluation code recorded in
tests/golden/eval_pairs.npz (tests/golden/gen_eval_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import eval_restatement as R
import tie_aware
from rdmnet_amd import _lib, evaluation
from rdmnet_amd import eval as cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_KEYS = ('ref_points_c', 'src_points_c', 'ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points',
             'src_corr_points', 'corr_scores', 'gt_node_corr_indices', 'gt_node_corr_overlaps', 'transform', 'estimated_transform')
THRESHOLDS = ('inlier_ratio', 'inlier_ratio_0.3', 'inlier_ratio_0.1', 'overlap')


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'eval_pairs.npz'))
    return {k: z[k] for k in z.files}


def pair_of(fx, name):
    return {k: fx[f'{name}/{k}'] for k in FILE_KEYS}


def reference_record(fx, name, nc, method='lgr'):
    """One record as rdm_eval_pairs lays it out, from the reference's recorded results (counts: ratio * n)."""
    p = f'{name}/nc{nc}/'
    ov, ir, ir3, ir1, res, n = fx[p + 'fine']
    err = fx[p + ('err_lgr' if method == 'lgr' else 'err_svd')]
    rec = np.zeros(_lib.EVAL_RECORD_WIDTH)
    rec[:12] = [n, res, ir, ir3, ir1, ov, fx[f'{name}/precision'], *err]
    return rec


def test_restatement_equals_the_reference(fx):
    """Selection, fine meters (every decided row), coarse precision, Procrustes and registration error of
    tests/eval_restatement.py against the reference's recorded results, every pair and --num_corr value."""
    for name in fx['names']:
        pair = pair_of(fx, name)
        for nc in fx['num_corrs']:
            p = f'{name}/nc{nc}/'
            for method in ('lgr', 'svd'):
                mine = R.evaluate(pair, method, int(nc) or None, float(fx['radius']))
                assert np.array_equal(mine['rows'], np.sort(fx[p + 'sel'])), (name, nc)
                ov, ir, ir3, ir1, res, n = fx[p + 'fine']
                assert mine['fine']['num_corr'] == n
                assert abs(mine['fine']['residual'] - res) < 1e-5  # (the reference's mean is fp32)
                for key, ratio in zip(THRESHOLDS, (ir, ir3, ir1, ov)):
                    m = mine['fine'][key]
                    assert m['lo'] <= round(ratio * n) <= m['lo'] + m['undecided'], (name, nc, key)
                    assert m['undecided'] <= 0.01 * n
                    i = THRESHOLDS.index(key)
                    assert (m['lo'], m['undecided']) == (fx[p + 'lo'][i], fx[p + 'undecided'][i])
                assert abs(mine['coarse'][3] - fx[f'{name}/precision']) < 1e-12
                want = fx[p + ('err_lgr' if method == 'lgr' else 'err_svd')]
                if method == 'lgr':
                    assert np.allclose(mine['registration'], want, rtol=0, atol=1e-9), (name, nc)
                else:  # DESIGN 7's LGR bounds, measured as there (tie_aware.rre_rte): 1e-3 degrees, 1e-4 m
                    rre, rte = tie_aware.rre_rte(mine['transform'], fx[p + 'svd_transform'])
                    assert rre < 1e-3 and rte < 1e-4, (name, nc, rre, rte)
                    assert fx[p + 'sigma_ratio'] > 1e-4


def test_select_keeps_the_lowest_rows_of_a_tie():
    scores = np.array([0.5, 0.9, 0.5, 0.5, 0.1, 0.9, 0.5], np.float32)
    assert R.select(scores, 4).tolist() == [0, 1, 2, 5]
    assert R.select(scores, 2).tolist() == [1, 5]
    assert R.select(scores, 7).tolist() == list(range(7)) and R.select(scores, None).tolist() == list(range(7))


def test_file_order_and_skip_rule(tmp_path):
    names = ['10_2_3', '2_10_11', '2_9_10', '8_15_16', '8_14_15', '9_0_1', 'b_1_2', 'a_10_11', 'a_9_10']
    for n in names:
        (tmp_path / (n + '.npz')).write_bytes(b'')
    (tmp_path / 'notes.txt').write_text('x')
    total, todo = cli.list_pairs(str(tmp_path))
    assert total == 9
    got = [(pos, os.path.basename(f)[:-4], ids) for pos, f, ids in todo]
    # eval.py:78-81: by the integers; 8_15_16 keeps its position in the count and is dropped (eval.py:94-95)
    assert got == [(1, '2_9_10', (2, 9, 10)), (2, '2_10_11', (2, 10, 11)), (3, '8_14_15', (8, 14, 15)), (5, '9_0_1', (9, 0, 1)),
                   (6, '10_2_3', (10, 2, 3)), (7, 'a_9_10', ('a', 9, 10)), (8, 'a_10_11', ('a', 10, 11)), (9, 'b_1_2', ('b', 1, 2))]


def test_arguments(capsys):
    p = cli.make_parser()
    a = p.parse_args(['--features-root', 'x'])
    assert (a.method, a.num_corr, a.verbose, a.test_epoch) == ('lgr', None, False, None)
    a = p.parse_args(['--features-root', 'x', '--method', 'ransac', '--num_corr', '250', '--verbose', '--batch', '8'])
    assert (a.method, a.num_corr, a.verbose, a.batch) == ('ransac', 250, True, 8)
    for bad in ('teaser', 'ransac_featurematch', 'icp'):
        with pytest.raises(SystemExit):
            p.parse_args(['--features-root', 'x', '--method', bad])
        assert bad in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(['--method', 'lgr'])  # no directory
    with pytest.raises(ValueError):
        _lib.EvalOptions.of('teaser')


def empty_meters_as_zero(line):
    """The reference's meters average no records to nan (np.mean of an empty list); Summary has always printed 0 there."""
    return re.sub(r'\bnan\b', '0.000', line)


@pytest.mark.parametrize('nc', [0, 250])
def test_report_and_pair_messages_match_the_reference(fx, nc):
    """Summary.commit_record + report_lines + eval.pair_message on the reference's recorded per-pair results reproduce every
    line eval_one_epoch logged for the same directory (method lgr, verbose)."""
    want = [str(s) for s in fx[f'lines/lgr/nc{nc}']]
    names = [str(n) for n in fx['names']] + [str(fx['skipped_name'])]
    order = sorted(names, key=lambda n: [int(i) for i in n.split('_')])
    summary = evaluation.Summary()
    got = []
    for pos, name in enumerate(order, 1):
        ids = tuple(int(i) for i in name.split('_'))
        if name == str(fx['skipped_name']):
            continue
        out = summary.commit_record(ids, reference_record(fx, name, nc))
        got.append(cli.pair_message(pos, len(order), ids, out))
    got += summary.report_lines()
    assert len(got) == len(want) == len(fx['names']) + 4
    assert got == [empty_meters_as_zero(w) for w in want]
    assert got[-4] == '  Node Detection, PRED_OV: 0.000, GT_OV: 0.000, PRED_T_OV: 0.000, GT_MAX_OV: 0.000'


def test_commit_record_equals_commit_of_measure(fx):
    """The record path adds to the meters what the host path adds (existing Summary.measure / commit)."""
    name = str(fx['names'][0])
    d = pair_of(fx, name)
    a, b = evaluation.Summary(), evaluation.Summary()
    nodes = (d['ref_points_c'], d['src_points_c'], d['ref_node_corr_indices'], d['src_node_corr_indices'], d['gt_node_corr_indices'])
    oa = a.update((0, 0, 1), d['transform'], d['estimated_transform'], d['ref_corr_points'], d['src_corr_points'], d['corr_scores'],
                  nodes)
    ob = b.commit_record((0, 0, 1), reference_record(fx, name, 0))
    assert set(oa) == set(ob) and a.meters.keys() == b.meters.keys()
    for k in oa:
        assert abs(float(oa[k]) - float(ob[k])) < 1e-5, k
    assert a.lines() == b.lines()
    assert len(evaluation.Summary().lines()) == 3  # (unchanged: the Node Detection line is report_lines' own)


def test_a_pair_without_correspondences_commits_no_fine_meters():
    rec = np.zeros(_lib.EVAL_RECORD_WIDTH)
    rec[1:6] = np.nan
    s = evaluation.Summary()
    out = s.commit_record((0, 1, 2), rec)
    assert 'f_IR' not in out and 'inlier_ratio' not in s.meters and s.meters['recall'] == [1.0]
    assert 'f_IR' not in cli.pair_message(1, 1, (0, 1, 2), out)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'rdmnet_hip.h')).read()
    L = _lib.lib()
    for n in ('rdm_eval_pairs', 'rdm_eval_pairs_workspace_bytes'):
        assert re.search(r'\b' + n + r'\s*\(', text) and hasattr(L, n) and n in _lib.SIGNATURES
    assert int(re.search(r'#define RDM_EVAL_RECORD_WIDTH (\d+)', text).group(1)) == _lib.EVAL_RECORD_WIDTH == len(_lib.EVAL_FIELDS)
    assert ctypes.sizeof(_lib.EvalOptions) == 40  # rdm_eval_options: 2 x i32, f64, f32, 3 x i32, u64
    assert L.rdm_abi_version() == 2
    # host-only: workspace sizes grow with the selection buffers and with RANSAC's scratch
    options = [_lib.EvalOptions.of('lgr'), _lib.EvalOptions.of('lgr', 1000), _lib.EvalOptions.of('ransac')]
    plain, limited, ransac = (L.rdm_eval_pairs_workspace_bytes(4, 4000, 1500, ctypes.addressof(o)) for o in options)
    assert 0 < plain < limited and ransac >= plain + L.rdm_ransac_workspace_bytes(50000)


def test_pack_eval_pairs_layout(fx):
    from rdmnet_amd import ops
    pairs = [pair_of(fx, str(n)) for n in fx['names'][:3]]
    packed = ops.pack_eval_pairs(pairs, pin=False)
    raw = packed.buf.numpy()

    def section(name):
        off, dtype, shape = packed.sections[name]
        return raw[off:off + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)

    assert all(off % 256 == 0 for off, _, _ in packed.sections.values())
    assert section('corr_offsets').tolist() == [0, 764, 764 + 409, 764 + 409 + 446]
    assert np.array_equal(section('ref_corr')[764:764 + 409], pairs[1]['ref_corr_points'])
    assert np.array_equal(section('gt_node_corr')[:len(pairs[0]['gt_node_corr_indices'])], pairs[0]['gt_node_corr_indices'])
    assert section('node_dims').tolist() == [[len(p['ref_points_c']), len(p['src_points_c'])] for p in pairs]
    assert np.array_equal(section('gt_transform')[2], pairs[2]['transform'])
