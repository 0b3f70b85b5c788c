"""GPU: rdm_information_matrix / rdm_engine_information_matrix through ops.information_matrix, ops.evaluate_registration,
Engine.information_matrix and `infer --information`, against the float64 restatement (tests/information_restatement.py) on the
inputs of tests/information_cases.py (tests/test_information.py asserts on the host that every row of them is decided).
The count and the correspondence set are equal.  Per entry |got - fsum| <= (C + 2) 2^-53 sum |terms|: the kernel adds the same
rounded products as the restatement, at most C - 1 additions deep per sum (each within 2^-53 of its partial sum, which the sum of
the absolute terms bounds), one more addition joins the two sums of a diagonal entry, and fsum itself rounds once."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import information_cases as cases
import information_restatement as I
from rdmnet_amd import _lib, config, engine, ops, weights

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(c, cell=None, source=None, target=None, radius=None):
    """-> (information numpy [6, 6], C, sum of d2, rows swept, corr numpy int64 [C, 2])"""
    info, n, sum_d2, swept, corr = ops._information(dev(c['source']) if source is None else source,
                                                    dev(c['target']) if target is None else target,
                                                    c['radius'] if radius is None else radius, c.get('s_transform'),
                                                    c.get('t_transform'), want_corr=True, cell=cell)
    assert info.dtype == torch.float64 and tuple(info.shape) == (6, 6) and not info.is_cuda
    assert corr.dtype == torch.int64 and corr.is_cuda and tuple(corr.shape) == (n, 2)
    return info.numpy(), n, sum_d2, swept, corr.cpu().numpy()


def check(name, c, got, want=None):
    want = want or I.information(c['source'], c['target'], c['radius'], c.get('s_transform'), c.get('t_transform'))
    info, n, sum_d2, swept, corr = got
    err = np.abs(info - want['information'])
    bound = (want['C'] + 2) * U * want['magnitude']
    print(name, 'C', n, 'of', len(c['source']), 'rows swept', swept, 'largest error / bound',
          float((err / np.where(bound > 0, bound, 1.0)).max()), 'largest error', float(err.max()))
    assert n == want['C'], name
    assert np.array_equal(corr, want['corr']), name
    assert (err <= bound).all(), (name, err, bound)
    assert np.array_equal(info, info.T) and np.array_equal(info[3:, 3:], n * np.eye(3)), name
    assert not np.signbit(info).any() or (info[np.signbit(info)] != 0).all(), name  # no negative zeros
    assert abs(sum_d2 - want['sum_d2']) <= (want['C'] + 1) * U * want['sum_d2'], name
    return want


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_cases_equal_the_restatement(name):
    c = cases.CASES[name]()
    want = check(name, c, run(c))
    if len(c['source']) == 0 or len(c['target']) == 0:
        assert want['C'] == 0 and not want['information'].any()
    if 'expect_C' in c:
        assert want['C'] == c['expect_C']
    info = ops.information_matrix(dev(c['source']), dev(c['target']), c['radius'], c.get('s_transform')) if 't_transform' not in c else None
    if info is not None:  # the public entry, Open3D's argument order, without the correspondences
        assert np.array_equal(info.numpy(), run(c)[0])


def test_a_pair_on_the_radius_is_outside_and_the_next_double_takes_it_in():
    c = cases.boundary()
    _, n, _, _, corr = run(c)
    assert n == 1 and corr.tolist() == [[1, 1]]
    wider = dict(c, radius=float(np.nextafter(c['radius'], 1.0)))
    got = run(wider)
    assert got[1] == 2 and got[4].tolist() == [[0, 0], [1, 1]]
    check('boundary, next double', wider, got)
    # nothing under the radius: the zero matrix
    info, n, sum_d2, _, corr = run(c, radius=0.125)
    assert n == 0 and not info.any() and sum_d2 == 0.0 and corr.shape == (0, 2)


def test_a_tie_goes_to_the_lower_target_row_and_the_matrix_shows_it():
    c = cases.tie()
    got = run(c)
    info, n, corr = got[0], got[1], got[4]
    lo, hi = c['tie_targets']
    assert [1, lo] in corr.tolist() and [1, hi] not in corr.tolist()
    want = check('tie', c, got)
    moved = I.R.moved(c['target'], c['t_transform'])
    other = want['corr'].copy()
    other[other[:, 0] == 1, 1] = hi
    wrong, magnitude = I.row_form(moved[other[:, 1]])
    assert (np.abs(info - wrong) > (n + 2) * U * magnitude).any()


def test_the_result_does_not_depend_on_the_cell_or_the_path():
    c = cases.CASES[cases.PATH_CASE]()
    n_q = len(c['source'])
    d2, _ = I.R.nearest(c['source'], c['target'])
    assert np.sqrt(d2.min()) > 4 * cases.PATH_CELLS['sweep']  # beyond the cube of 5^3 cells: nothing settles there
    runs = {name: run(c, cell) for name, cell in cases.PATH_CELLS.items()}
    for name, got in runs.items():
        print(name, 'rows swept', got[3])
        assert np.array_equal(got[0], runs['auto'][0]) and got[1] == runs['auto'][1] and got[2] == runs['auto'][2], name  # the same bits
        assert np.array_equal(got[4], runs['auto'][4]), name
    assert runs['sweep'][3] == n_q and runs['one_cell'][3] == 0  # the paths really differed
    check('path', c, runs['auto'])


def test_both_transforms_rows_of_four_and_two_calls():
    c = cases.moved_both()
    first = run(c)
    want = check('moved_both', c, first)
    assert 0 < want['C'] < len(c['source'])
    again = run(c)
    assert np.array_equal(first[0], again[0]) and first[1:4] == again[1:4] and np.array_equal(first[4], again[4])
    rng = np.random.default_rng(2)
    s4 = dev(np.concatenate([c['source'], rng.standard_normal((len(c['source']), 1)).astype(np.float32)], 1))
    t4 = dev(np.concatenate([c['target'], rng.standard_normal((len(c['target']), 1)).astype(np.float32)], 1))
    for a, b in ((s4, t4), (s4[:, :3], t4[:, :3]), (s4, dev(c['target']))):  # xyzi rows and a strided view of them
        got = run(c, source=a, target=b)
        assert np.array_equal(first[0], got[0]) and first[1:3] == got[1:3] and np.array_equal(first[4], got[4])


def raw_call(source, target, radius, s_transform=None, capacity=None):
    """rdm_information_matrix on sentinel-filled outputs -> (return code, out_host numpy [40], corr numpy [capacity, 2])."""
    L = _lib.lib()
    sd, td = dev(source), dev(target)
    capacity = len(source) if capacity is None else capacity
    corr = torch.full((max(capacity, 1), 2), -7, dtype=torch.int64, device='cuda')
    ws = torch.empty((L.rdm_information_workspace_bytes(len(source), len(target)),), dtype=torch.uint8, device='cuda')
    host = (ctypes.c_double * 40)(*([-7.0] * 40))
    rc = L.rdm_information_matrix(sd.data_ptr(), len(source), 3, td.data_ptr(), len(target), 3,
                                  0 if s_transform is None else s_transform.ctypes.data, 0, 0.0, float(radius), host, corr.data_ptr(),
                                  capacity, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, np.array(list(host)), corr.cpu().numpy()


def test_bad_points_and_radii_are_argument_errors_and_leave_the_outputs():
    c = cases.CASES['65x1025']()
    a, b = c['source'], c['target']
    bad_a, bad_b, inf_b = a.copy(), b.copy(), b.copy()
    bad_a[17, 1] = np.nan
    bad_b[1000, 2] = np.nan
    inf_b[5, 0] = np.inf
    inf_t = np.eye(4)
    inf_t[0, 3] = np.inf
    for q, s, t, r, text in ((bad_a, b, None, 0.6, 'not finite'), (a, bad_b, None, 0.6, 'not finite'), (a, inf_b, None, 0.6, 'not finite'),
                             (a, b, inf_t, 0.6, 'not finite'), (a, b, None, 0.0, 'radius'), (a, b, None, -1.0, 'radius'),
                             (a, b, None, float('nan'), 'radius')):
        rc, host, corr = raw_call(q, s, r, t)
        assert rc == -1 and text in _lib.lib().rdm_last_error().decode(), (rc, text)
        assert (host == -7.0).all() and (corr == -7).all()
    with pytest.raises(RuntimeError, match='not finite'):
        ops.information_matrix(dev(bad_a), dev(b), 0.6)
    with pytest.raises(ValueError):
        ops.information_matrix(dev(a), dev(b), 0.0)
    with pytest.raises(ValueError):
        ops.evaluate_registration(dev(a), dev(b), -0.6)
    # the next valid call succeeds; a capacity one short of C is the capacity error and writes no row beyond it
    want = I.information(a, b, 0.6)
    rc, host, corr = raw_call(a, b, 0.6)
    assert rc == 0 and host[36] == want['C'] and host[39] == 0.0 and np.array_equal(corr[:want['C']], want['corr'])
    assert (corr[want['C']:] == -7).all() and want['C'] > 1
    full = host.copy()
    rc, host, corr = raw_call(a, b, 0.6, capacity=want['C'] - 1)
    assert rc == -4 and 'capacity' in _lib.lib().rdm_last_error().decode()
    assert np.array_equal(host, full) and np.array_equal(corr, want['corr'][:want['C'] - 1])
    rc, host, corr = raw_call(a, b, 0.6, capacity=want['C'])
    assert rc == 0 and np.array_equal(corr, want['corr'])


def test_evaluate_registration_equals_alignment_quality_and_the_restatement():
    c = cases.one_transform()
    source, target, S = c['source'], c['target'], c['s_transform']
    res = ops.evaluate_registration(dev(source), dev(target), 0.6, S)
    want = I.information(source, target, 0.6, S)
    quality = ops.alignment_quality(dev(target), dev(source), S, 0.6)  # (ref, src): its src side is this call's source
    print(res, quality)
    assert isinstance(res, ops.RegistrationResult) and res.num_correspondences == want['C'] and res.iterations == 0
    assert abs(res.fitness - quality['fitness_src']) <= 1e-12 * quality['fitness_src'] and res.fitness == want['C'] / len(source)
    assert abs(res.inlier_rmse - quality['inlier_rmse_src']) <= 1e-12 * quality['inlier_rmse_src'] and res.inlier_rmse > 0
    assert np.array_equal(res.correspondence_set.cpu().numpy(), want['corr']) and np.array_equal(res.transformation, S)
    info, corr = ops.information_matrix(dev(source), dev(target), 0.6, S, return_correspondences=True)
    assert torch.equal(info, res.information) and torch.equal(corr, res.correspondence_set)
    check('evaluate', dict(source=source, target=target, radius=0.6, s_transform=S),
          (info.numpy(), res.num_correspondences, want['sum_d2'], 0, corr.cpu().numpy()), want)
    empty = ops.evaluate_registration(dev(source[:0]), dev(target), 0.6)
    assert empty.fitness == 0.0 and empty.inlier_rmse == 0.0 and empty.correspondence_set.shape == (0, 2)
    assert np.array_equal(empty.transformation, np.eye(4))


@pytest.fixture(scope='module')
def state():
    return weights.synthetic_state_dict(config.make_cfg(), seed=0)


def crop_pair(scans, r=9.0):
    def crop(p):
        return p[np.linalg.norm(p[:, :2], axis=1) < r]
    return crop(scans['s000000']), crop(scans['s000004'])


def level_points(eng, res):
    t = {k: eng.tensor(k) for k in ('points0', 'nodes')}
    n0, m_r = int(res.level_ref_sizes[0]), int(res.n_ref_nodes)
    return {'input': (t['points0'][:n0].contiguous(), t['points0'][n0:].contiguous()),
            'coarse': (t['nodes'][:m_r].contiguous(), t['nodes'][m_r:].contiguous())}


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_engine_entry_equals_the_op_on_the_resident_clouds(state, scans):
    cfg = config.make_cfg()
    ref, src = crop_pair(scans)
    T = np.array([[0.99995, -0.01, 0, 0.1], [0.01, 0.99995, 0, -0.05], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float64)
    eng = engine.Engine(cfg, state)
    with pytest.raises(RuntimeError, match='no completed forward run'):
        eng.information_matrix()
    eng.keep_taps(True)
    res = eng.run(dev(ref), dev(src))
    used, own, before = int(res.arena_used), eng.transform(), [x.clone() for x in eng.corr()]
    for level, (rp, sp) in level_points(eng, res).items():
        for transform, radius in ((None, 0.6), (T, 0.6), (T, 2.0)):
            got = eng.information_matrix(transform, radius, level, return_correspondences=True)
            want = ops.information_matrix(sp, rp, radius, own if transform is None else transform, return_correspondences=True)
            print(level, radius, 'C', got[1].shape[0], 'of', sp.shape[0])
            assert same(got, want) and eng.information_corr == want[1].shape[0], level  # (the same bits)
            assert torch.equal(eng.information_matrix(transform, radius, level), want[0])
        assert 0 < want[1].shape[0] <= sp.shape[0]
    rp, sp = level_points(eng, res)['input']
    assert torch.equal(eng.information_matrix(), ops.information_matrix(sp, rp, cfg.fine_matching.acceptance_radius, own))
    with pytest.raises(ValueError):
        eng.information_matrix(T, 0.6, 'middle')
    with pytest.raises(ValueError):
        eng.information_matrix(T, 0.0)
    # the run's outputs and the arena are as before; the other entries on the last run still work
    assert np.array_equal(eng.transform(), own) and all(torch.equal(x, y) for x, y in zip(eng.corr(), before))
    assert eng.alignment_quality(T, 0.6)['n_src'] == sp.shape[0]
    assert int(eng.run(dev(ref), dev(src)).arena_used) == used


def test_engine_entry_after_a_lock_step_group(state, scans, golden_dir):
    cfg = config.make_cfg()
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    eng = engine.Engine(cfg, state)
    group = [engine.Engine(cfg, None, share_with=eng) for _ in range(2)]
    for e in group:
        e.keep_taps(True)
    clouds = [tuple(dev(x) for x in crop_pair(scans)), (dev(z['ref0']), dev(z['src0']))]
    with torch.cuda.stream(torch.cuda.Stream()):
        results = engine.Engine.run_lockstep(group, clouds)
        for e, res, (r, s) in zip(group, results, clouds):
            rp, sp = level_points(e, res)['input']
            assert rp.shape == r.shape and sp.shape == s.shape
            got = e.information_matrix(return_correspondences=True)
            assert same(got, ops.information_matrix(sp, rp, cfg.fine_matching.acceptance_radius, e.transform(), return_correspondences=True))
            assert got[1].shape[0] > 0
        torch.cuda.current_stream().synchronize()


def test_harness_adds_the_information_keys_and_nothing_else(tmp_path):
    runs = {}
    for name, flags in (('plain', []), ('information', ['--information'])):
        out_dir = tmp_path / name
        cmd = [sys.executable, '-m', 'rdmnet_amd.infer', '--synthetic', '2', '--synthetic-distinct', '2', '--synthetic-cache',
               str(tmp_path / 'pairs'), '--out', str(out_dir), '--pairs-in-flight', '1', '--no-ransac'] + flags
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        files = sorted(glob.glob(str(out_dir / '*.npz')))
        assert len(files) == 2
        runs[name] = ([dict(np.load(fn)) for fn in files], [x for x in p.stdout.splitlines() if x.startswith('seq_id')])
    keys = {'information', 'information_corr'}
    for plain, with_i, line, plain_line in zip(runs['plain'][0], runs['information'][0], runs['information'][1], runs['plain'][1]):
        assert set(with_i) == set(plain) | keys and not keys & set(plain)
        for k in plain:
            assert np.array_equal(plain[k], with_i[k]), k
        info, n = with_i['information'], with_i['information_corr']
        assert info.dtype == np.float64 and info.shape == (6, 6) and n.dtype == np.int64 and n.shape == ()
        assert line == plain_line + f', info_corr: {int(n)}' and 'info_corr' not in plain_line
        want, corr = ops.information_matrix(dev(with_i['src_points']), dev(with_i['ref_points']), 0.6, with_i['estimated_transform'],
                                            return_correspondences=True)
        assert np.array_equal(info, want.numpy()) and int(n) == corr.shape[0] > 0
