"""GPU: rdm_nearest / rdm_realign_error / rdm_engine_alignment_quality through ops.get_nearest_neighbor,
ops.compute_modified_chamfer_distance, ops.compute_registration_rmse, ops.alignment_quality, Engine.alignment_quality and
`infer --quality`, against the reference's recorded outputs (tests/golden/nearest.npz) and the float64 restatement
(tests/nearest_restatement.py).  Indices are equal and d2 is bit-equal to the restatement everywhere (the same expression on the
same doubles); against the reference distances agree to 1e-9 m: coordinates are at most a few hundred metres in float64, so a
moved coordinate carries about 1e-13 of round-off, and the fixture's generator asserts that every row is decided."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nearest_restatement as R
from rdmnet_amd import _lib, config, engine, ops, weights

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'nearest.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def pairs(golden_dir):
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    return {k: z[k] for k in z.files}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def grid_points(rng, n, lo, hi):
    """n points with coordinates on the 2^-6 grid in [lo, hi): differences, squares and their sums are exact in double."""
    return (rng.integers(int(lo * 64), int(hi * 64), size=(n, 3)) / 64.0).astype(np.float32)


def nearest(q, s, q_transform=None, s_transform=None, cell=None, radius=0.0):
    """-> (idx int64 numpy, d2 float64 numpy, (sum of distances, rows within radius, their sum of d2, rows swept))"""
    idx, d2, totals = ops._nearest(q if isinstance(q, torch.Tensor) else dev(q), s if isinstance(s, torch.Tensor) else dev(s),
                                   q_transform, s_transform, cell, radius)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and idx.is_cuda and d2.is_cuda
    return idx.cpu().numpy().astype(np.int64), d2.cpu().numpy(), totals


def check(q, s, q_transform=None, s_transform=None, cells=(None,), where=''):
    """Indices equal and d2 bit-equal to the restatement at every cell edge -> the restatement's (d2, idx)."""
    want_d2, want_idx = R.nearest(q, s, q_transform, s_transform)
    for cell in cells:
        idx, d2, totals = nearest(q, s, q_transform, s_transform, cell)
        print(where, 'n_q', len(q), 'n_s', len(s), 'cell', cell, 'rows swept', totals[3])
        assert np.array_equal(idx, want_idx), (where, cell, np.nonzero(idx != want_idx)[0][:8])
        assert np.array_equal(d2, want_d2), (where, cell)
    return want_d2, want_idx


def test_fixture_cases_equal_the_reference(fx, pairs, scans):
    for p in fx['pairs']:
        ref, src = pairs[f'ref{p}'], pairs[f'src{p}']
        for name in ('gt', 'off'):
            tag = f'p{p}/{name}'
            gt, est = fx[f'{tag}/gt'], fx[f'{tag}/est']
            dist, idx = ops.get_nearest_neighbor(dev(ref), dev(src), True, s_transform=est)
            assert dist.dtype == torch.float64 and idx.dtype == torch.int64 and dist.shape == idx.shape == (len(ref),)
            assert np.array_equal(idx.cpu().numpy(), fx[f'{tag}/idx'].astype(np.int64)), tag
            err = float(np.abs(dist.cpu().numpy() - fx[f'{tag}/dist']).max())
            print(tag, 'largest distance error', err)
            assert err <= 1e-9, tag
            assert torch.equal(ops.get_nearest_neighbor(dev(ref), dev(src), s_transform=est), dist)
            scalars_equal_the_reference(fx, tag, ref, ref, src, gt, est)
    scalars_equal_the_reference(fx, 'scans', scans['s000000'], scans['s000000'], scans['s000004'], fx['scans/gt'], fx['scans/est'])


def scalars_equal_the_reference(fx, tag, raw, ref, src, gt, est):
    for r in fx['radii']:
        _, _, totals = nearest(ref, src, None, est, None, float(r))
        assert totals[1] / len(ref) == float(fx[f'{tag}/overlap{r}']), (tag, r)
    chamfer = ops.compute_modified_chamfer_distance(dev(raw), dev(ref), dev(src), gt, est)
    rmse = ops.compute_registration_rmse(dev(src), gt, est)
    print(tag, 'chamfer', chamfer, float(fx[f'{tag}/chamfer']), 'rmse', rmse, float(fx[f'{tag}/rmse']))
    assert isinstance(chamfer, float) and abs(chamfer - float(fx[f'{tag}/chamfer'])) <= 1e-9, tag
    assert isinstance(rmse, float) and abs(rmse - float(fx[f'{tag}/rmse'])) <= 1e-9, tag


CELLS = (None, 0.01, 0.5, 1.0, 3.0, 1000.0)


def test_ties_go_to_the_lowest_index():
    rng = np.random.default_rng(0)
    # a support cloud with duplicated rows, shuffled: every duplicate pair is an exact tie for the queries at and around it
    base = grid_points(rng, 400, -2.0, 2.0)
    s = np.concatenate([base, base[:150], base[:40]])
    s = s[rng.permutation(len(s))]
    q = np.concatenate([base[:200], grid_points(rng, 100, -2.5, 2.5)])
    d2, idx = check(q, s, cells=CELLS, where='duplicates')
    assert (d2[:200] == 0).all()
    first = np.array([np.nonzero((s == p).all(axis=1))[0][0] for p in q[:200]])
    assert np.array_equal(idx[:200], first)
    # an integer lattice queried at the cell centres: eight equidistant corners
    g = np.arange(6, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    lattice = lattice[rng.permutation(len(lattice))]
    c = np.arange(5, dtype=np.float32) + np.float32(0.5)
    centres = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    d2, idx = check(centres, lattice, cells=CELLS, where='lattice')
    assert (d2 == 0.75).all()
    for i in (0, 57, 124):
        corners = np.nonzero((np.abs(lattice - centres[i]) == 0.5).all(axis=1))[0]
        assert len(corners) == 8 and idx[i] == corners.min()
    # a query equidistant from points in two different cells (cell edge 0.5: x = 0.25 lies in cell 0, x = -0.25 in cell -1),
    # the lower row in either of them
    far = grid_points(rng, 20, 5.0, 6.0)
    for first_x in (0.25, -0.25):
        s2 = np.concatenate([np.float32([[first_x, 0, 0], [-first_x, 0, 0]]), far])
        d2, idx = check(np.zeros((1, 3), np.float32), s2, cells=(0.5, None, 0.1, 2.0), where='two cells')
        assert idx.tolist() == [0] and d2.tolist() == [0.0625]
        d2, idx = check(np.zeros((1, 3), np.float32), s2[::-1].copy(), cells=(0.5, None, 0.1, 2.0), where='two cells reversed')
        assert idx.tolist() == [len(s2) - 2]


def test_the_result_does_not_depend_on_the_cell_or_the_path():
    """3 000 x 3 000: a dense cluster, a sparse halo and one support point 5 km away.  Support coordinates are multiples of 1/64,
    query coordinates odd multiples of 1/128, so every distance is at least sqrt(3)/128 = 0.0135 m: with a cell edge of 0.004 m
    the cube phase 1 searches reaches at most 0.012 m and settles nothing; with an edge of 10^5 m the support is one cell."""
    rng = np.random.default_rng(1)

    def cloud():
        return np.concatenate([grid_points(rng, 2000, 20.0, 21.0), grid_points(rng, 999, 0.0, 40.0), np.float32([[5000.0, 3.0, 7.0]])])
    s = cloud()
    q = cloud() + np.float32(1.0 / 128.0)
    order = rng.permutation(3000)
    s, q = s[order], q[rng.permutation(3000)]
    want_d2, want_idx = R.nearest(q, s)
    assert np.sqrt(want_d2.min()) >= 0.0135
    runs = {name: nearest(q, s, cell=cell, radius=0.25) for name, cell in (('auto', None), ('small', 0.004), ('large', 1e5))}
    for name, (idx, d2, totals) in runs.items():
        print(name, 'rows swept', totals[3], 'sums', totals[:3])
        assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2), name
        assert totals[:3] == runs['auto'][2][:3], name  # (float equality: the same bits)
    assert runs['small'][2][3] == 3000 and runs['large'][2][3] == 0
    assert 0 < runs['auto'][2][1] < 3000  # the radius separates rows
    near = np.sqrt(want_d2) < 0.25
    assert runs['auto'][2][1] == int(near.sum())
    assert abs(runs['auto'][2][0] - np.sqrt(want_d2).sum()) <= 1e-12 * np.sqrt(want_d2).sum()
    again = nearest(q, s, radius=0.25)
    assert np.array_equal(again[0], runs['auto'][0]) and np.array_equal(again[1], runs['auto'][1]) and again[2] == runs['auto'][2]


@pytest.mark.parametrize('n_s', [1, 63, 64, 65, 1025])
def test_wavefront_and_tile_boundaries(n_s):
    rng = np.random.default_rng(10 + n_s)
    s = grid_points(rng, n_s, -3.0, 3.0)
    q = np.concatenate([grid_points(rng, 120, -3.0, 3.0), s[:10], grid_points(rng, 10, -900.0, 900.0)])  # (far outside the box too)
    check(q, s, cells=(None, 0.01, 0.7, 100.0), where=f'n_s={n_s}')


def test_empty_clouds_rows_of_four_and_transforms():
    rng = np.random.default_rng(3)
    s, q = grid_points(rng, 300, -3.0, 3.0), grid_points(rng, 257, -4.0, 4.0)
    e = np.zeros((0, 3), np.float32)
    idx, d2, totals = nearest(e, s, radius=1.0)
    assert idx.shape == d2.shape == (0,) and totals == (0.0, 0, 0.0, 0)
    dist, idx = ops.get_nearest_neighbor(dev(q), dev(e), True)
    assert dist.shape == (257,) and torch.isinf(dist).all() and (dist > 0).all() and (idx == 0).all() and idx.dtype == torch.int64
    assert ops.get_nearest_neighbor(dev(e), dev(e)).shape == (0,)
    want_d2, want_idx = check(q, s, where='plain')
    # xyzi rows (row stride 4) and a strided view of them
    q4 = dev(np.concatenate([q, rng.standard_normal((len(q), 1)).astype(np.float32)], 1))
    s4 = dev(np.concatenate([s, rng.standard_normal((len(s), 1)).astype(np.float32)], 1))
    for a, b in ((q4, s4), (q4[:, :3], s4[:, :3]), (q4, dev(s))):
        idx, d2, _ = nearest(a, b)
        assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)
    # a transform on the query, on the support, on both (a general rotation: the moved coordinates round)
    a = 0.3
    T = np.array([[np.cos(a), -np.sin(a), 0, 0.5], [np.sin(a), np.cos(a), 0, -1.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float64)
    U = np.array([[1, 0, 0, 0.1], [0, np.cos(0.2), -np.sin(0.2), 0], [0, np.sin(0.2), np.cos(0.2), -0.3], [0, 0, 0, 1]], np.float64)
    for qt, st in ((T, None), (None, T), (T, U), (torch.from_numpy(U), np.eye(4))):
        check(q, s, qt, st, cells=(None, 0.05, 50.0), where='transform')
    # the identity is the cloud as it is
    idx, d2, _ = nearest(q, s, np.eye(4), np.eye(4))
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)


def raw_call(q, s, q_transform=None, s_transform=None):
    """rdm_nearest on caller-filled outputs -> (return code, idx, d2)."""
    L = _lib.lib()
    qd, sd = dev(q), dev(s)
    idx = torch.full((len(q),), -7, dtype=torch.int32, device='cuda')
    d2 = torch.full((len(q),), -7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty((L.rdm_nearest_workspace_bytes(len(q), len(s)),), dtype=torch.uint8, device='cuda')
    totals = (ctypes.c_double * 5)()
    rc = L.rdm_nearest(qd.data_ptr(), len(q), 3, sd.data_ptr(), len(s), 3, 0 if q_transform is None else q_transform.ctypes.data,
                       0 if s_transform is None else s_transform.ctypes.data, 0.0, 0.0, idx.data_ptr(), d2.data_ptr(), totals,
                       ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), d2.cpu().numpy()


def test_non_finite_points_are_an_argument_error_and_leave_the_outputs():
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((100, 3)).astype(np.float32), rng.standard_normal((90, 3)).astype(np.float32)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[17, 1] = np.nan
    bad_b[5, 2] = np.nan
    inf_t = np.eye(4)
    inf_t[0, 3] = np.inf
    for q, s, qt, st in ((bad_a, b, None, None), (a, bad_b, None, None), (a, b, inf_t, None), (a, b, None, inf_t)):
        rc, idx, d2 = raw_call(q, s, qt, st)
        assert rc == -1 and 'not finite' in _lib.lib().rdm_last_error().decode()
        assert (idx == -7).all() and (d2 == -7.0).all()
        with pytest.raises(RuntimeError, match='not finite'):
            ops.get_nearest_neighbor(dev(q), dev(s), q_transform=qt, s_transform=st)
        with pytest.raises(RuntimeError, match='not finite'):
            ops.alignment_quality(dev(q), dev(s), st if st is not None else qt, 0.5)
    with pytest.raises(RuntimeError, match='not finite'):
        ops.compute_registration_rmse(dev(bad_a), np.eye(4), np.eye(4))
    with pytest.raises(RuntimeError, match='not finite'):
        ops.compute_registration_rmse(dev(a), inf_t, np.eye(4))
    rc, idx, d2 = raw_call(a, b)  # the next valid call succeeds
    want_d2, want_idx = R.nearest(a, b)
    assert rc == 0 and np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)
    assert ops.compute_registration_rmse(dev(a), np.eye(4), np.eye(4)) == 0.0


def test_alignment_quality_of_a_constructed_pair():
    """A rigid copy (an exact quarter turn and translation) with 10 % outliers; some rows shifted by grid steps so that the
    inlier distances are not all zero."""
    rng = np.random.default_rng(5)
    ref = grid_points(rng, 1000, -4.0, 4.0)
    T = np.array([[0, -1, 0, 0.5], [1, 0, 0, -1.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float64)
    copy = ref[:900] + (rng.integers(-3, 4, size=(900, 3)) / 64.0).astype(np.float32) * (rng.random((900, 1)) < 0.5)
    src = np.concatenate([R.moved(copy, np.linalg.inv(T)).astype(np.float32), grid_points(rng, 100, 30.0, 40.0)])
    assert np.array_equal(R.moved(src[:900], T), copy.astype(np.float64))  # exact
    for radius in (0.3, 0.05):
        got, want = ops.alignment_quality(dev(ref), dev(src), T, radius), R.alignment_quality(ref, src, T, radius)
        print(radius, got)
        assert got['n_ref'] == 1000 and got['n_src'] == 1000
        for side in ('ref', 'src'):
            assert got[f'fitness_{side}'] == want[f'fitness_{side}'] and 0.5 < got[f'fitness_{side}'] < 1.0
            assert abs(got[f'inlier_rmse_{side}'] - want[f'inlier_rmse_{side}']) <= 1e-12 * want[f'inlier_rmse_{side}']
            assert want[f'inlier_rmse_{side}'] > 0
        assert abs(got['chamfer'] - want['chamfer']) <= 1e-12 * want['chamfer']
    assert got['fitness_src'] <= 0.9
    # a radius exactly on a pair's distance is decided strictly
    ref2 = np.float32([[0, 0, 0], [10, 0, 0]])
    src2 = np.float32([[0.5, 0, 0], [10.25, 0, 0]])
    on = ops.alignment_quality(dev(ref2), dev(src2), None, 0.5)
    above = ops.alignment_quality(dev(ref2), dev(src2), None, float(np.nextafter(0.5, 1.0)))
    assert on['fitness_ref'] == on['fitness_src'] == 0.5 and on['inlier_rmse_ref'] == 0.25 and on['chamfer'] == 0.75
    assert above['fitness_ref'] == above['fitness_src'] == 1.0
    assert on == R_public(R.alignment_quality(ref2, src2, None, 0.5))
    none = ops.alignment_quality(dev(ref2), dev(src2), None, 0.125)
    assert none['fitness_ref'] == 0.0 and none['inlier_rmse_ref'] == 0.0 and none['inlier_rmse_src'] == 0.0
    with pytest.raises(ValueError):
        ops.alignment_quality(dev(ref2), dev(src2), None, 0.0)


def R_public(d):
    return {k: v for k, v in d.items() if not k.startswith('n_within')}


@pytest.fixture(scope='module')
def state():
    return weights.synthetic_state_dict(config.make_cfg(), seed=0)


def crop_pair(scans, r=9.0):
    def crop(p):
        return p[np.linalg.norm(p[:, :2], axis=1) < r]
    return crop(scans['s000000']), crop(scans['s000004'])


def level_points(eng, res):
    t = {k: eng.tensor(k) for k in ('points0', 'points1', 'nodes')}
    n0, nf, m_r = int(res.level_ref_sizes[0]), int(res.level_ref_sizes[1]), int(res.n_ref_nodes)
    return {'input': (t['points0'][:n0].contiguous(), t['points0'][n0:].contiguous()),
            'fine': (t['points1'][:nf].contiguous(), t['points1'][nf:].contiguous()),
            'coarse': (t['nodes'][:m_r].contiguous(), t['nodes'][m_r:].contiguous())}


def test_engine_entry_equals_the_op_at_all_three_levels(state, scans):
    cfg = config.make_cfg()
    ref, src = crop_pair(scans)
    T = np.array([[0.99995, -0.01, 0, 0.1], [0.01, 0.99995, 0, -0.05], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float64)
    plain = engine.Engine(cfg, state)  # never calls it
    with pytest.raises(RuntimeError, match='no completed forward run'):
        plain.alignment_quality()
    plain.run(dev(ref), dev(src))
    untouched = (plain.transform(), [x.clone() for x in plain.corr()])
    eng = engine.Engine(cfg, state)
    eng.keep_taps(True)
    res = eng.run(dev(ref), dev(src))
    used = int(res.arena_used)
    own = eng.transform()
    for level, (rp, sp) in level_points(eng, res).items():
        for transform, radius in ((None, 0.6), (T, 0.6), (T, 2.0)):
            got = eng.alignment_quality(transform, radius, level)
            want = ops.alignment_quality(rp, sp, own if transform is None else transform, radius)
            print(level, got)
            assert got == want and got['n_ref'] == rp.shape[0] and got['n_src'] == sp.shape[0], level  # (floats: the same bits)
    rp, sp = level_points(eng, res)['input']
    assert rp.shape[0] == len(ref)
    assert eng.alignment_quality() == ops.alignment_quality(rp, sp, own, cfg.fine_matching.acceptance_radius)
    with pytest.raises(ValueError):
        eng.alignment_quality(T, 0.6, 'middle')
    with pytest.raises(ValueError):
        eng.alignment_quality(T, 0.0)
    # the run's outputs are those of a run that never calls it, before and after; the other entries on the last run still work
    assert np.array_equal(own, untouched[0]) and all(torch.equal(x, y) for x, y in zip(eng.corr(), untouched[1]))
    assert eng.gt_point_correspondences(T, 0.6, 'fine').shape[0] > 0
    res2 = eng.run(dev(ref), dev(src))
    assert int(res2.arena_used) == used
    assert np.array_equal(eng.transform(), untouched[0]) and all(torch.equal(x, y) for x, y in zip(eng.corr(), untouched[1]))
    assert plain.alignment_quality(T, 0.6, 'fine') == eng.alignment_quality(T, 0.6, 'fine')  # (no taps needed)


def test_engine_entry_after_a_lock_step_group(state, scans, pairs):
    cfg = config.make_cfg()
    eng = engine.Engine(cfg, state)
    group = [engine.Engine(cfg, None, share_with=eng) for _ in range(2)]
    for e in group:
        e.keep_taps(True)
    clouds = [tuple(dev(x) for x in crop_pair(scans)), (dev(pairs['ref0']), dev(pairs['src0']))]
    alone = []
    for r, s in clouds:
        eng.run(r, s)
        alone.append((eng.transform(), [x.clone() for x in eng.corr()]))
    with torch.cuda.stream(torch.cuda.Stream()):
        results = engine.Engine.run_lockstep(group, clouds)
        for e, res, (r, s), (T, corr) in zip(group, results, clouds, alone):
            rp, sp = level_points(e, res)['input']
            assert rp.shape == r.shape and sp.shape == s.shape
            got = e.alignment_quality()
            assert got == ops.alignment_quality(rp, sp, e.transform(), cfg.fine_matching.acceptance_radius)
            assert np.array_equal(e.transform(), T) and all(torch.equal(x, y) for x, y in zip(e.corr(), corr))
        torch.cuda.current_stream().synchronize()


def test_harness_adds_the_quality_keys_and_nothing_else(tmp_path):
    runs = {}
    for name, flags in (('plain', []), ('quality', ['--quality'])):
        out_dir = tmp_path / name
        cmd = [sys.executable, '-m', 'rdmnet_amd.infer', '--synthetic', '2', '--synthetic-distinct', '2', '--synthetic-cache',
               str(tmp_path / 'pairs'), '--out', str(out_dir), '--pairs-in-flight', '1', '--no-ransac'] + flags
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        files = sorted(glob.glob(str(out_dir / '*.npz')))
        assert len(files) == 2
        runs[name] = ([dict(np.load(fn)) for fn in files], [x for x in p.stdout.splitlines() if x.startswith('seq_id')])
    keys = {f'quality_{k}' for k in ops.QUALITY_KEYS}
    assert len(keys) == 5
    for plain, with_q, line, plain_line in zip(runs['plain'][0], runs['quality'][0], runs['quality'][1], runs['plain'][1]):
        assert set(with_q) == set(plain) | keys and not keys & set(plain)
        for k in plain:
            assert np.array_equal(plain[k], with_q[k]), k
        for k in ops.QUALITY_KEYS:
            v = with_q[f'quality_{k}']
            assert v.dtype == np.float64 and v.shape == () and np.isfinite(v)
            assert f'{k}: {float(v):.4f}' in line, line
        assert 0.0 < float(with_q['quality_fitness_ref']) <= 1.0 and float(with_q['quality_chamfer']) > 0.0
        assert line.startswith(plain_line) and 'fitness' not in plain_line
        want = ops.alignment_quality(dev(with_q['ref_points']), dev(with_q['src_points']), with_q['estimated_transform'], 0.6)
        assert all(float(with_q[f'quality_{k}']) == want[k] for k in ops.QUALITY_KEYS)
