"""GPU: rdm_ball_count / rdm_ball_fill through ops.get_correspondences, ops.compute_overlap, ops.overlap_labels,
Engine.gt_point_correspondences and `prepare overlap`, against the reference's recorded outputs (tests/golden/pair_overlap.npz) and
the float64 restatement (tests/pair_overlap_restatement.py).  Lists, counts, order and overlaps are exact everywhere: the fixture's
generator asserts that no pair lies within 1e-9 relative of the radius, and the synthetic cases below use coordinates on a 2^-6
grid with power-of-two radii, so every d2 is exact in double."""
import os

import numpy as np
import pytest
import torch

import pair_overlap_restatement as R
from rdmnet_amd import config, engine, ops, prepare, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'pair_overlap.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def pairs(golden_dir):
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    return {k: z[k] for k in z.files}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def check_against_restatement(ref, src, T, r, where=''):
    """List, overlaps (both sides) and labels of (ref, src, T, r) against the restatement; -> the restatement's result."""
    q = R.ball_query(ref, src, T, r)
    got = ops.get_correspondences(dev(ref), dev(src), T, r)
    assert got.dtype == torch.int64 and got.is_cuda and got.dim() == 2 and got.shape[1] == 2
    got = got.cpu().numpy()
    print(where, 'N', len(ref), 'M', len(src), 'C', len(q['corr']), 'longest row', int(q['counts'].max()) if len(ref) else 0)
    assert got.shape == q['corr'].shape and np.array_equal(got, q['corr']), where
    want = (R._fraction(q['ref_min_d2'], r), R._fraction(q['src_min_d2'], r))
    assert ops.compute_overlap(dev(ref), dev(src), T, r, both=True) == want, where
    assert ops.compute_overlap(dev(ref), dev(src), T, r) == want[0], where
    lr, ls = ops.overlap_labels(dev(ref), dev(src), T, r)
    assert lr.dtype == ls.dtype == torch.bool and lr.shape == (len(ref),) and ls.shape == (len(src),)
    assert np.array_equal(lr.cpu().numpy(), np.isin(np.arange(len(ref)), q['corr'][:, 0])), where
    assert np.array_equal(ls.cpu().numpy(), np.isin(np.arange(len(src)), q['corr'][:, 1])), where
    return q


def test_fixture_cases_equal_the_reference(fx, pairs):
    for p in fx['pairs']:
        ref, src, T = pairs[f'ref{p}'], pairs[f'src{p}'], pairs[f'T{p}']
        for r in fx['radii']:
            want = fx[f'p{p}/r{r}/corr'].astype(np.int64)
            got = ops.get_correspondences(dev(ref), dev(src), T, float(r))
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (p, r)
            o_ref, o_src = ops.compute_overlap(dev(ref), dev(src), T, float(r), both=True)
            print('pair', p, 'r', r, 'C', len(want), 'overlap', o_ref, o_src)
            assert isinstance(o_ref, float) and o_ref == float(fx[f'p{p}/r{r}/overlap']), (p, r)
            assert o_src == float(fx[f'p{p}/r{r}/overlap_src']), (p, r)
            lr, ls = ops.overlap_labels(dev(ref), dev(src), T, float(r))
            assert np.array_equal(lr.cpu().numpy(), np.isin(np.arange(len(ref)), want[:, 0])), (p, r)
            assert np.array_equal(ls.cpu().numpy(), np.isin(np.arange(len(src)), want[:, 1])), (p, r)


def test_two_point_boundary_case(fx):
    ref, src, r = dev(fx['two_point/ref']), dev(fx['two_point/src']), float(fx['two_point/radius'])
    assert ops.get_correspondences(ref, src, None, r).cpu().numpy().tolist() == fx['two_point/corr'].tolist() == [[0, 0]]  # closed
    assert ops.compute_overlap(ref, src, None, r, both=True) == (float(fx['two_point/overlap']),) * 2 == (0.0, 0.0)    # strict
    lr, ls = ops.overlap_labels(ref, src, None, r)
    assert lr.tolist() == [True] and ls.tolist() == [True]
    assert ops.compute_overlap(ref, src, None, float(np.nextafter(r, 1.0)), both=True) == (1.0, 1.0)
    assert ops.get_correspondences(ref, src, None, float(np.nextafter(r, 0.0))).shape == (0, 2)


def test_empty_inputs():
    rng = np.random.default_rng(0)
    a, e = rng.standard_normal((300, 3)).astype(np.float32), np.zeros((0, 3), np.float32)
    far = a + np.float32(100.0)
    for ref, src in ((e, a), (a, e), (e, e), (a, far)):
        got = ops.get_correspondences(dev(ref), dev(src), None, 0.6)
        assert got.shape == (0, 2) and got.dtype == torch.int64 and got.is_cuda
        assert ops.compute_overlap(dev(ref), dev(src), None, 0.6, both=True) == (0.0, 0.0)
        lr, ls = ops.overlap_labels(dev(ref), dev(src), None, 0.6)
        assert lr.shape == (len(ref),) and ls.shape == (len(src),) and not lr.any() and not ls.any()


def grid_points(rng, n, lo, hi):
    """n points with coordinates on the 2^-6 grid in [lo, hi): differences, squares and their sums are exact in double."""
    return (rng.integers(int(lo * 64), int(hi * 64), size=(n, 3)) / 64.0).astype(np.float32)


def test_long_rows_come_out_complete_and_ordered():
    """One ref point with 3 000 src points of ONE cell within r of it (exact duplicates among them, in shuffled row order), other
    ref rows around it, some of which see the same crowd: rows of thousands next to rows of a few and empty rows."""
    rng = np.random.default_rng(1)
    r = 0.5  # cell edge 0.5 (1 + 1e-6): the crowd lies in the cell [0, 0.5)^3
    crowd = grid_points(rng, 2800, 0.0, 0.25)
    crowd = np.concatenate([crowd, crowd[:200]])  # exact duplicate points under different row numbers
    sparse = grid_points(rng, 500, -3.0, 3.0)
    src = np.concatenate([crowd, sparse])
    src = src[rng.permutation(len(src))]
    ref = np.concatenate([grid_points(rng, 40, -3.0, 3.0), np.float32([[0.125, 0.125, 0.125]]), grid_points(rng, 30, -0.5, 0.75),
                          grid_points(rng, 40, -3.0, 3.0)])
    q = check_against_restatement(ref, src, None, r, 'long rows')
    assert q['counts'][40] >= 3000 and (q['counts'] == 0).any() and ((q['counts'] > 0) & (q['counts'] < 64)).any()
    row = q['corr'][q['corr'][:, 0] == 40][:, 1]
    assert (np.diff(row) > 0).all()


@pytest.mark.parametrize('n', [1, 257])
def test_geometry_of_the_index(n):
    """Negative coordinates, points exactly on cell faces, ref rows outside the src box, block edges (N = 257: two workgroups of
    the point kernels and a partial one of the row kernels; N = 1), xyzi input, transform None against the identity, and a
    rigid transform."""
    rng = np.random.default_rng(100 + n)
    r = 0.5
    faces = (rng.integers(-6, 7, size=(120, 3)) * 0.5).astype(np.float32)  # multiples of r: on (or within 1e-6 of) cell faces
    src = np.concatenate([grid_points(rng, 400, -3.0, 3.0), faces])
    inside = np.concatenate([grid_points(rng, 150, -3.0, 3.0), (rng.integers(-6, 7, size=(60, 3)) * 0.5).astype(np.float32)])
    outside = np.concatenate([grid_points(rng, 30, 3.0, 3.5), grid_points(rng, 17, -40.0, 40.0)])  # beside and far outside the box
    ref = np.concatenate([inside, outside])[rng.permutation(257)][:n]
    if n == 1:
        ref = src[7:8] + np.float32([0.25, 0, 0])
    q = check_against_restatement(ref, src, None, r, f'geometry n={n}')
    assert len(q['corr']) > 0
    # xyzi rows (stride 4) and a strided view; None against the identity
    ref4 = dev(np.concatenate([ref, rng.standard_normal((len(ref), 1)).astype(np.float32)], 1))
    src4 = dev(np.concatenate([src, rng.standard_normal((len(src), 1)).astype(np.float32)], 1))
    want = torch.from_numpy(q['corr']).cuda()
    assert torch.equal(ops.get_correspondences(ref4, src4, None, r), want)
    assert torch.equal(ops.get_correspondences(ref4[:, :3], src4[:, :3], np.eye(4), r), want)
    assert torch.equal(ops.get_correspondences(dev(ref), dev(src), torch.eye(4), r), want)
    # swapped roles (M = n), and a rigid transform with an exactly representable rotation (a quarter turn) and translation
    check_against_restatement(src, ref, None, r, f'geometry swapped n={n}')
    T = np.array([[0, -1, 0, 0.5], [1, 0, 0, -1.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float64)
    moved_back = (R.moved(src, np.linalg.inv(T))).astype(np.float32)  # exact: grid coordinates, a quarter turn
    qt = check_against_restatement(ref, moved_back, T, r, f'geometry transform n={n}')
    assert np.array_equal(qt['corr'], q['corr'])


def test_two_calls_give_identical_results(pairs):
    ref, src, T = dev(pairs['ref3'][:6000]), dev(pairs['src3'][:6000]), pairs['T3']
    a, b = ops.get_correspondences(ref, src, T, 0.6), ops.get_correspondences(ref, src, T, 0.6)
    assert a.shape[0] > 0 and torch.equal(a, b)
    assert ops.compute_overlap(ref, src, T, 0.6, both=True) == ops.compute_overlap(ref, src, T, 0.6, both=True)
    for s, t in zip(ops.overlap_labels(ref, src, T, 0.6), ops.overlap_labels(ref, src, T, 0.6)):
        assert torch.equal(s, t)


def test_non_finite_points_raise_the_librarys_error():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((100, 3)).astype(np.float32), rng.standard_normal((90, 3)).astype(np.float32)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[17, 1] = np.nan
    bad_b[5, 2] = np.inf
    for ref, src, T in ((bad_a, b, None), (a, bad_b, None), (a, b, np.full((4, 4), np.nan))):
        with pytest.raises(RuntimeError, match='not finite'):
            ops.get_correspondences(dev(ref), dev(src), T, 0.6)
    with pytest.raises(RuntimeError, match='not finite'):
        ops.compute_overlap(dev(a), dev(b * np.float32(1e12)), None, 0.6)  # beyond 2^30 cells of 0.6 m
    assert ops.get_correspondences(dev(a), dev(b), None, 0.6).shape[0] == len(R.get_correspondences(a, b, None, 0.6))  # still usable


@pytest.fixture(scope='module')
def state():
    return weights.synthetic_state_dict(config.make_cfg(), seed=0)


def crop_pair(scans, r=9.0):
    def crop(p):
        return p[np.linalg.norm(p[:, :2], axis=1) < r]
    return crop(scans['s000000']), crop(scans['s000004'])


def test_engine_entry_equals_the_op_at_all_three_levels(state, scans):
    cfg = config.make_cfg()
    ref, src = crop_pair(scans)
    T = np.array([[0.99995, -0.01, 0, 0.1], [0.01, 0.99995, 0, -0.05], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float64)
    eng = engine.Engine(cfg, state)
    eng.keep_taps(True)
    res = eng.run(dev(ref), dev(src))
    used = int(res.arena_used)
    t = {k: eng.tensor(k) for k in ('points0', 'points1', 'nodes')}
    n0, nf, m_r = int(res.level_ref_sizes[0]), int(res.level_ref_sizes[1]), int(res.n_ref_nodes)
    assert n0 == len(ref)
    levels = {'input': (t['points0'][:n0], t['points0'][n0:], 0.3), 'fine': (t['points1'][:nf], t['points1'][nf:], 0.6),
              'coarse': (t['nodes'][:m_r], t['nodes'][m_r:], 4.0)}
    for level, (rp, sp, radius) in levels.items():
        for transform in (T, None):
            got = eng.gt_point_correspondences(transform, radius, level)
            want = ops.get_correspondences(rp.contiguous(), sp.contiguous(), transform, radius)
            print(level, 'points', rp.shape[0], sp.shape[0], 'correspondences', want.shape[0])
            assert want.shape[0] > 0 and got.dtype == torch.int64 and torch.equal(got, want), level
    with pytest.raises(ValueError):
        eng.gt_point_correspondences(T, 0.6, 'middle')
    with pytest.raises(ValueError):
        eng.gt_point_correspondences(T, 0.0, 'fine')
    # the other entries on the last run still work after it, and a plain engine (no taps) gives the same lists
    after = eng.feature_correspondences('fine', 'mutual')
    plain = engine.Engine(cfg, state)
    with pytest.raises(RuntimeError, match='no completed forward run'):
        plain.gt_point_correspondences(T, 0.6)
    plain.run(dev(ref), dev(src))
    assert torch.equal(plain.gt_point_correspondences(T, 0.6, 'fine'), eng.gt_point_correspondences(T, 0.6, 'fine'))
    assert torch.equal(plain.feature_correspondences('fine', 'mutual')['ref_corr_indices'], after['ref_corr_indices'])
    # a forward that does not call it is what it was: a second run of the engine that called it takes the same arena and gives
    # the same result as the run before the calls
    first = (eng.transform(), [x.clone() for x in eng.corr()])
    res2 = eng.run(dev(ref), dev(src))
    assert int(res2.arena_used) == used
    assert np.array_equal(eng.transform(), first[0]) and all(torch.equal(x, y) for x, y in zip(eng.corr(), first[1]))


def test_prepare_overlap_writes_the_expected_lines(tmp_path):
    rng = np.random.default_rng(4)
    scans = {0: grid_points(rng, 500, -2.0, 2.0), 3: grid_points(rng, 450, -2.0, 2.0), 9: grid_points(rng, 300, -1.0, 3.0)}
    os.makedirs(tmp_path / 'downsampled_xyzi' / '08')
    os.makedirs(tmp_path / 'icp10')
    for frame, p in scans.items():
        np.save(tmp_path / 'downsampled_xyzi' / '08' / ('%06d.npy' % frame),
                np.concatenate([p, np.ones((len(p), 1), np.float32)], 1))
    T = np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 0.125], [0, 0, 0, 1]], np.float64)
    with open(tmp_path / 'icp10' / '08', 'w') as f:  # `anc pos` + the pose: frame0 = pos is the ref, frame1 = anc the src
        f.write(prepare.format_pair_line(0, 3, T))
        f.write(prepare.format_pair_line(3, 9, np.eye(4)))
    assert prepare.main(['overlap', '--dataset-root', str(tmp_path), '--radius', '0.5']) == 0
    lines = open(tmp_path / 'overlap10' / '08').read().splitlines()
    want = []
    for (src_frame, ref_frame), transform in (((0, 3), T), ((3, 9), np.eye(4))):
        q = R.ball_query(scans[ref_frame], scans[src_frame], transform, 0.5)
        want.append(prepare.format_overlap_line(ref_frame, src_frame, R._fraction(q['ref_min_d2'], 0.5),
                                                R._fraction(q['src_min_d2'], 0.5), len(q['corr'])).rstrip('\n'))
        assert len(q['corr']) > 0
    assert lines == want
