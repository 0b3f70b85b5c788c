"""GPU: rdm_feature_match / ops.feature_match / Engine.feature_correspondences / `infer --feature-match` / `eval --method
ransac_featurematch` against the reference's recorded outputs (tests/golden/feature_match.npz) and the float64 restatement
(tests/feature_match_restatement.py).  Indices and order are exact everywhere; distances within 1 fp32 ulp."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_match_restatement as R
from rdmnet_amd import _lib, config, engine, eval as cli, evaluation, ops, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MODES = {'nearest': {}, 'mutual': {'mutual': True}, 'bilateral': {'bilateral': True}}


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'feature_match.npz'))
    return {k: z[k] for k in z.files}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def check_both_sides(a, b, fast=False, where=''):
    """feature_nearest(both_sides) on (a, b) against the restatement, both directions; -> the lines that took phase 2."""
    nn_ab, d_ab, nn_ba, d_ba, phase2 = ops.feature_nearest(dev(a), dev(b), both_sides=True, return_phase2=True)
    ref = R.nearest_fast if fast else R.nearest
    for got_i, got_d, (want_i, want_d), side in ((nn_ab, d_ab, ref(a, b), 'rows'), (nn_ba, d_ba, ref(b, a), 'columns')):
        got_i, got_d = got_i.cpu().numpy(), got_d.cpu().numpy()
        bad = np.nonzero(got_i != want_i)[0]
        ulps = R.ulp_diff(got_d, want_d)
        print(where, side, 'lines', len(want_i), 'wrong', len(bad), 'max ulp', int(ulps.max()) if len(ulps) else 0)
        assert got_i.dtype == np.int64 and len(bad) == 0, (where, side, bad[:8], got_i[bad[:8]], want_i[bad[:8]])
        assert len(ulps) == 0 or ulps.max() <= 1, (where, side)
    p2 = phase2.cpu().numpy()
    print(where, 'phase-2 lines', p2.tolist(), 'of', (a.shape[0], b.shape[0]))
    # one side only gives the same rows
    one = ops.feature_nearest(dev(a), dev(b))
    assert torch.equal(one[0], nn_ab) and torch.equal(one[1].view(torch.int32), d_ab.view(torch.int32)) and one[2] is None
    return p2


@pytest.mark.parametrize('tag', ['crop9', 'small', 'random'])
@pytest.mark.parametrize('mode', list(MODES))
def test_fixture_cases_equal_the_reference(fx, tag, mode):
    rf, sf = dev(fx[f'{tag}/ref_feats']), dev(fx[f'{tag}/src_feats'])
    ri, si = ops.feature_match(rf, sf, **MODES[mode])
    assert ri.dtype == si.dtype == torch.int64 and ri.is_cuda
    assert np.array_equal(ri.cpu().numpy(), fx[f'{tag}/{mode}/ref_corr_indices'])
    assert np.array_equal(si.cpu().numpy(), fx[f'{tag}/{mode}/src_corr_indices'])
    if mode != 'bilateral':
        rc, sc, dist = ops.feature_correspondences(dev(fx[f'{tag}/ref_points']), dev(fx[f'{tag}/src_points']), rf, sf,
                                                   mutual=mode == 'mutual', return_feat_dist=True)
        assert np.array_equal(rc.cpu().numpy(), fx[f'{tag}/{mode}/ref_corr_points'])
        assert np.array_equal(sc.cpu().numpy(), fx[f'{tag}/{mode}/src_corr_points'])
        ulps = R.ulp_diff(dist.cpu().numpy(), fx[f'{tag}/{mode}/feat_dists'])
        print(tag, mode, 'distance max ulp', int(ulps.max()))
        assert ulps.max() <= 1
    else:  # (the reference's extract_correspondences_from_feats has no bilateral: against the restatement)
        out = ops.feature_correspondences(dev(fx[f'{tag}/ref_points']), dev(fx[f'{tag}/src_points']), rf, sf, bilateral=True,
                                          return_feat_dist=True)
        want = R.correspondences(fx[f'{tag}/ref_points'], fx[f'{tag}/src_points'], fx[f'{tag}/ref_feats'], fx[f'{tag}/src_feats'],
                                 bilateral=True, return_feat_dist=True)
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
        assert R.ulp_diff(out[2].cpu().numpy(), want[2]).max() <= 1


@pytest.mark.parametrize('n,m,c', [(1, 1, 1), (3, 65, 1), (65, 129, 86), (300, 257, 256), (129, 1, 256)])
def test_shapes_that_break_tiles(n, m, c):
    rng = np.random.default_rng(n * 1000 + m)
    a, b = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((m, c)).astype(np.float32)
    check_both_sides(a, b, where=f'{n}x{m}x{c}')
    # a strided view (row stride above c, not a multiple of 4): the scalar-load path
    wide = dev(np.concatenate([a, np.zeros((n, 3), np.float32)], 1))
    got = ops.feature_nearest(wide[:, :c], dev(b))[0]
    assert np.array_equal(got.cpu().numpy(), R.nearest(a, b)[0])


def test_2048_normal_features():
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal((2048, 256)).astype(np.float32), rng.standard_normal((2048, 256)).astype(np.float32)
    check_both_sides(a, b, fast=True, where='2048x2048x256')


def test_degenerate_sizes():
    a, b = torch.zeros((0, 32), device='cuda'), torch.randn((5, 32), device='cuda')
    for kw in ({}, {'mutual': True}):
        ri, si = ops.feature_match(a, b, **kw)
        assert ri.shape == si.shape == (0,) and ri.dtype == torch.int64
    assert [t.shape[0] for t in ops.feature_correspondences(torch.zeros((0, 3), device='cuda'), torch.zeros((5, 3), device='cuda'), a, b,
                                                            return_feat_dist=True)] == [0, 0, 0]
    with pytest.raises(RuntimeError, match='m = 0'):
        ops.feature_match(b, a)
    with pytest.raises(RuntimeError, match='m = 0'):
        ops.feature_match(a, a)
    with pytest.raises(RuntimeError, match='c = 1025'):
        ops.feature_match(torch.zeros((2, 1025), device='cuda'), torch.zeros((2, 1025), device='cuda'))


def near_tie_case():
    """64 rows of a (entries multiples of 2^-10, |a|^2 about 20, column 1 zero) whose two nearest rows of b are a_i + d e0 and
    a_i + d (1 + 2^-20) e1, d = 2^-6: squared distances 2^-12 and 2^-12 (1 + 2^-20)^2, 4.7e-10 apart -- far below the fp32
    expansion's round-off at |a|^2 + |b|^2 = 40 --, the nearer one at the HIGHER index, in the same or the next column tile."""
    rng = np.random.default_rng(11)
    n, m, c = 64, 640, 256
    a = (np.round(rng.standard_normal((n, c)) * 0.28 * 1024) / 1024).astype(np.float32)
    a[:, 1] = 0
    b = (np.round(rng.standard_normal((m, c)) * 0.28 * 1024) / 1024).astype(np.float32)
    d = np.float32(2.0 ** -6)
    far = np.array([128 * (i % 4) + i // 4 for i in range(n)])
    near = np.array([128 * (i % 4 + (i // 16) % 2) + 64 + i // 4 for i in range(n)])
    assert len(set(far) | set(near)) == 2 * n and (near > far).all() and near.max() < m
    for i in range(n):
        b[far[i]] = a[i]
        b[far[i], 1] = d * np.float32(1 + 2.0 ** -20)
        b[near[i]] = a[i]
        b[near[i], 0] = a[i, 0] + d
        assert np.float64(b[near[i], 0]) == np.float64(a[i, 0]) + 2.0 ** -6 and np.float64(b[far[i], 1]) == 2.0 ** -6 + 2.0 ** -26
    return a, b, near


def test_near_ties_the_expansion_cannot_decide():
    a, b, near = near_tie_case()
    want = R.nearest(a, b)[0]
    assert np.array_equal(want, near)  # the float64 answer is the higher index
    p2 = check_both_sides(a, b, where='near ties, rows')
    assert p2[0] == 64  # every such line went through the float64 pass
    p2 = check_both_sides(b, a, where='near ties, columns')  # roles swapped: the same lines as columns
    assert p2[1] == 64


def test_exact_ties_take_the_lowest_index():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((200, 64)).astype(np.float32), rng.standard_normal((400, 64)).astype(np.float32)
    b[70] = b[5]
    b[300] = b[5]     # another tile
    b[399] = b[140]
    a[0] = b[5]
    a[1] = b[5] + np.float32(0.01) * rng.standard_normal(64).astype(np.float32)
    a[150] = b[140]
    a[199] = a[3]     # duplicated rows of a: the column side
    a[130] = a[3]
    b[17] = a[3] + np.float32(0.01) * rng.standard_normal(64).astype(np.float32)
    nn_ab, _, nn_ba, _ = ops.feature_nearest(dev(a), dev(b), both_sides=True)
    assert nn_ab[0] == 5 and nn_ab[1] == 5 and nn_ab[150] == 140 and nn_ba[17] == 3
    check_both_sides(a, b, where='exact ties')


def test_two_calls_give_identical_bits():
    rng = np.random.default_rng(3)
    a, b = dev(rng.standard_normal((700, 128)).astype(np.float32)), dev(rng.standard_normal((900, 128)).astype(np.float32))
    x, y = ops.feature_nearest(a, b, both_sides=True), ops.feature_nearest(a, b, both_sides=True)
    for s, t in zip(x, y):
        assert torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)


@pytest.fixture(scope='module')
def state():
    return weights.synthetic_state_dict(config.make_cfg(), seed=0)


def crop_pair(scans, r=9.0):
    def crop(p):
        return p[np.linalg.norm(p[:, :2], axis=1) < r]
    return crop(scans['s000000']), crop(scans['s000004'])


def test_engine_entry_equals_the_op_on_the_runs_exported_tensors(state, scans):
    cfg = config.make_cfg()
    ref, src = crop_pair(scans)
    eng = engine.Engine(cfg, state)
    eng.keep_taps(True)
    res = eng.run(dev(ref), dev(src))
    t = {k: eng.tensor(k) for k in ('points1', 'decoder', 'nodes', 'feats_c')}
    nf, m_r, D = int(res.level_ref_sizes[1]), int(res.n_ref_nodes), cfg.backbone.output_dim
    levels = {'fine': (t['points1'][:nf], t['points1'][nf:], t['decoder'][:nf, :D], t['decoder'][nf:, :D]),
              'coarse': (t['nodes'][:m_r], t['nodes'][m_r:], t['feats_c'][:m_r], t['feats_c'][m_r:])}
    for level, (rp, sp, rf, sf) in levels.items():
        for mode, kw in MODES.items():
            got = eng.feature_correspondences(level, mode, return_phase2=True)
            ri, si = ops.feature_match(rf, sf, **kw)
            rc, sc, dist = ops.feature_correspondences(rp, sp, rf, sf, return_feat_dist=True, **kw)
            assert torch.equal(got['ref_corr_indices'], ri) and torch.equal(got['src_corr_indices'], si), (level, mode)
            assert torch.equal(got['ref_corr_points'], rc) and torch.equal(got['src_corr_points'], sc), (level, mode)
            assert torch.equal(got['feat_dists'].view(torch.int32), dist.view(torch.int32)), (level, mode)
            assert ri.shape[0] > 0
            print(level, mode, 'correspondences', ri.shape[0], 'phase-2 lines', got['phase2_lines'], 'of', (rf.shape[0], sf.shape[0]))
    with pytest.raises(ValueError):
        eng.feature_correspondences('middle')
    with pytest.raises(ValueError):
        eng.feature_correspondences('fine', 'ratio')


def test_engine_entry_without_taps_and_without_a_forward(state, scans):
    cfg = config.make_cfg()
    eng = engine.Engine(cfg, state)
    with pytest.raises(RuntimeError, match='no completed forward run'):
        eng.feature_correspondences()
    ref, src = crop_pair(scans)
    eng.run(dev(ref), dev(src))  # keep-taps off: the four tensors stay in the arena, so the call works
    plain = eng.feature_correspondences('fine', 'mutual')
    eng2 = engine.Engine(cfg, state)
    eng2.keep_taps(True)
    eng2.run(dev(ref), dev(src))
    taps = eng2.feature_correspondences('fine', 'mutual')
    assert plain['ref_corr_indices'].shape[0] > 0
    for k in plain:
        assert torch.equal(plain[k], taps[k]), k


def test_harness_writes_the_five_keys_and_eval_reads_them(tmp_path, capsys):
    out_dir = tmp_path / 'out'
    cmd = [sys.executable, '-m', 'rdmnet_amd.infer', '--synthetic', '2', '--synthetic-distinct', '2', '--synthetic-cache',
           str(tmp_path / 'pairs'), '--gt-nodes', '--out', str(out_dir), '--feature-match', 'mutual', '--pairs-in-flight', '1']
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    files = sorted(glob.glob(str(out_dir / '*.npz')))
    assert len(files) == 2
    logged = [x for x in p.stdout.splitlines() if 'feat_IR' in x]
    assert len(logged) == 2, p.stdout[-2000:]
    pairs = []
    for fn, line in zip(sorted(files, key=cli.sort_key), logged):
        z = np.load(fn)
        assert set(z.files) == set(evaluation.TEST_NPZ_KEYS) | {'transform'} | set(evaluation.FEATURE_MATCH_KEYS), fn
        n = z['feat_corr_dists'].shape[0]
        assert n > 0 and z['feat_ref_corr_points'].shape == z['feat_src_corr_points'].shape == (n, 3)
        assert z['feat_ref_corr_indices'].dtype == np.int64 and (np.diff(z['feat_ref_corr_indices']) > 0).all()  # mutual: ascending
        assert np.array_equal(z['feat_ref_corr_points'], z['ref_points_f'][z['feat_ref_corr_indices']])
        assert np.array_equal(z['feat_src_corr_points'], z['src_points_f'][z['feat_src_corr_indices']])
        ir = evaluation.evaluate_correspondences(z['feat_ref_corr_points'], z['feat_src_corr_points'], z['transform'].astype(np.float64),
                                                 positive_radius=0.6)['inlier_ratio']
        assert f'nFeatCorr: {n}, feat_IR: {ir:.3f}' in line, (line, n, ir)
        pairs.append(z)
    # eval --method ransac_featurematch: the estimator of --method ransac on the descriptor rows
    args = cli.make_parser(own_methods=True).parse_args(['--features-root', str(out_dir), '--method', 'ransac_featurematch', '--num_corr', '50',
                                         '--verbose'])
    summary = cli.evaluate(args, emit=lambda s: None)
    records, transforms = ops.evaluate_pairs([cli.load_pair(fn, 'ransac_featurematch') for fn in sorted(files, key=cli.sort_key)],
                                             'ransac', 50)
    assert summary is not None
    for z, rec, T in zip(pairs, records, transforms):
        scores = -z['feat_corr_dists']
        order = np.lexsort((np.arange(len(scores)), -scores))[:50]  # the 50 smallest distances, lowest rows among equals
        rows = np.sort(order)
        want = ops.ransac_correspondences(dev(z['feat_src_corr_points'][rows]), dev(z['feat_ref_corr_points'][rows]), 0.3, 4, 50000,
                                          seed=0)[0].cpu().numpy()
        assert np.array_equal(np.asarray(T, np.float32).reshape(4, 4), want)
        named = dict(zip(_lib.EVAL_FIELDS, rec))
        assert named['num_corr'] == min(50, len(scores))
