"""GPU: the rigid-fit solver of csrc/procrustes.h inside each of its five clients, on the degenerate and edge geometry of
rigid_fit_cases.py, against the float64 SVD reference and the criteria A to D stated there (test_rigid_fit.py shows that the
reference, and its float32 rounding, meet them).  Every test prints its worst figure per criterion.

Worst figures of one MI355X run are in DESIGN.md 7 (every one at least a factor of two inside its bound, most at the level of the
float32-rounded reference)."""
import numpy as np
import pytest
import torch

import eval_restatement
import icp_restatement
import lgr_options_restatement
import rigid_fit_cases as C
import robust_restatement as RR
from test_rigid_fit import RANSAC_ITERATIONS, RANSAC_SEEDS, RANSAC_THRESHOLD, ransac_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def cuda32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def report(name, worst):
    print(name, 'worst:', {k: f'{v:.2e}' for k, v in sorted(worst.items())})


# ---------------------------------------------------------------------------------------------------------------- eval svd
def eval_pair(src, ref, scores):
    z = np.zeros(1, np.int64)
    return {'ref_corr_points': np.asarray(ref, np.float32).reshape(-1, 3), 'src_corr_points': np.asarray(src, np.float32).reshape(-1, 3),
            'corr_scores': np.asarray(scores, np.float32).reshape(-1), 'transform': np.eye(4, dtype=np.float32),
            'ref_node_corr_indices': z, 'src_node_corr_indices': z, 'gt_node_corr_indices': np.zeros((1, 2), np.int64), 'node_dims': (2, 2)}


def test_eval_svd_on_every_family_size_and_weight_pattern(ops):
    """One pair per (family, size, weight pattern), the near-tie away from the origin and an empty pair, in ONE batched call
    (scored rule, fp32 out).  A, B, C, D per pair; the last row of T is 0 0 0 1; an all-zero-score pair and the empty pair
    return exactly the identity."""
    entries = []
    for family in C.FAMILIES:
        for n in C.sizes_of(family):
            case = C.make(family, n)
            for pattern in C.PATTERNS:
                entries.append((f'{case.name}/{pattern}', case, C.scores_of(pattern, case.n), pattern))
    tie = C.tie_case((16.0, -8.0, 4.0))
    entries.append(('mirrored_tie/offset', tie, np.ones(6, np.float32), 'uniform'))
    pairs = [eval_pair(c.src, c.ref, s) for _, c, s, _ in entries] + [eval_pair(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))]
    records, transforms = ops.evaluate_pairs(pairs, 'svd')
    assert transforms.shape == (len(pairs), 4, 4) and transforms.dtype == np.float32
    worst, classes = {}, {'ABC': 0, 'AB': 0, 'ABD': 0}
    for (name, case, scores, pattern), T in zip(entries, transforms):
        fit = case.fit('scored', scores)
        m = C.check(T, fit, 'fp32', where=name, worst=worst.setdefault(case.family, {}))
        classes[m['applies']] += 1
        assert np.array_equal(T[3], [0, 0, 0, 1]), name
        if pattern == 'zero':
            assert fit.zero and np.array_equal(T, np.eye(4, dtype=np.float32)), (name, T)
    assert np.array_equal(transforms[-1], np.eye(4, dtype=np.float32))
    assert min(classes.values()) > 0, classes
    for family, w in worst.items():
        report(f'eval svd {family}', w)
    print('pairs per class', classes)


def test_eval_svd_num_corr_fits_the_selected_rows(ops):
    """--num_corr 250 on 257-row cases: the fit is that of the rows eval_restatement.select selects."""
    worst = {}
    for family in ('noisy', 'coplanar', 'collinear', 'mirrored'):
        case = C.make(family, 257)
        scores = C.scores_of('uniform', 257)
        rows = eval_restatement.select(scores, 250)
        assert len(rows) == 250
        records, transforms = ops.evaluate_pairs([eval_pair(case.src, case.ref, scores)], 'svd', 250)
        C.check(transforms[0], case.fit('scored', scores, rows=rows), 'fp32', where=family, worst=worst)
        if family == 'noisy':  # the seven rows left out move the solution by more than the bound: the comparison can tell
            assert C.measure(transforms[0], case.fit('scored', scores), 'fp32')['trans'] > 1e-5
    report('eval svd num_corr 250', worst)


# --------------------------------------------------------------------------------------------------------------------- ICP
ICP_RADIUS = 0.05


def near_motion(case):
    """The case's motion followed by a turn of 0.01 degrees about the target's centroid and a shift of 0.2 mm."""
    c = case.ref.astype(np.float64).mean(0)
    a = np.radians(0.01)
    u = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    Rs = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    init = np.eye(4)
    init[:3, :3] = Rs @ case.motion[:3, :3]
    init[:3, 3] = Rs @ (case.motion[:3, 3] - c) + c + [2e-4, -1e-4, 1e-4]
    return init


def icp_first_update(ops, src, tgt, radius, init, where):
    """One ICP iteration -> (update U as 3x4, the reference's fit of the moved source onto its correspondences).  Asserts that
    the device's correspondences are the restatement's."""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    pcd = src.astype(np.float64) if init is None else icp_restatement.apply(init, src.astype(np.float64))
    idx, d2, near = icp_restatement.Target(tgt, radius).correspondences(pcd)
    got_idx, got_d2 = ops.icp_correspondences(torch.from_numpy(pcd).cuda(), cuda32(tgt), radius)
    assert np.array_equal(got_idx.cpu().numpy(), idx) and (idx >= 0).all(), where
    res = ops.icp_point_to_point(cuda32(src), cuda32(tgt), radius, init=init, max_iteration=1, history=True)
    assert res.iterations == 1 and res.history.shape == (2, 15) and res.history[0, 2] == len(src), where
    fit = C.Fit(pcd, tgt.astype(np.float64)[idx], 'plain')
    return res.history[0, 3:15].reshape(3, 4), fit, idx, float(np.sqrt(d2.max())), res


@pytest.mark.parametrize('family', ['full', 'coplanar', 'near_coplanar', 'collinear', 'half_turn', 'exact', 'far', 'two'])
def test_icp_update_of_one_iteration(ops, family):
    """Source = the target moved back by the case's motion, init within 0.01 degrees / 0.2 mm of it: every row's nearest
    neighbour is its own (asserted on the device and in the restatement, the smallest spacing above twice the residual).
    The update of history[0] against the fit of the restatement's moved source, fp64 bounds (plain rule)."""
    from scipy.spatial import cKDTree
    worst = {}
    for n in C.sizes_of(family):
        case = C.make(family, n)
        U, fit, idx, residual, res = icp_first_update(ops, case.src, case.ref, ICP_RADIUS, near_motion(case), case.name)
        assert np.array_equal(idx, np.arange(case.n)), case.name
        spacing = cKDTree(case.ref.astype(np.float64)).query(case.ref.astype(np.float64), k=2)[0][:, 1].min()
        assert spacing > 2 * residual and residual < ICP_RADIUS, (case.name, spacing, residual)
        fit.family = family
        m = C.check(U, fit, 'fp64', where=case.name, worst=worst)
        assert m['applies'] == ('AB' if family in ('collinear', 'two') else 'ABC'), (case.name, m)
    report(f'icp {family}', worst)


@pytest.mark.parametrize('family,n', [('single', 1), ('one_point', 3), ('one_point', 65), ('one_point', 257), ('exact_one_point', 64)])
def test_icp_update_from_one_point_is_the_identity_and_the_centroid_shift(ops, family, n):
    """H == 0 exactly (one correspondence, or every source row equal and so every row matched to the first target): criterion D
    on the update -- the identity, and the translation the difference of the centroids."""
    case = C.make(family, n)
    tgt = (case.src.astype(np.float64) + [0.25, -0.125, 0.0625]).astype(np.float32)
    U, fit, idx, residual, res = icp_first_update(ops, case.src, tgt, 1.0, None, case.name)
    assert fit.zero and (idx == 0).all()
    m = C.check(U, fit, 'fp64', where=case.name)
    assert m['applies'] == 'ABD' and np.array_equal(U[:, 3], tgt[0].astype(np.float64) - case.src[0].astype(np.float64))
    assert np.array_equal(res.transformation[:3], U)


def test_icp_second_iteration_on_exact_data_changes_nothing(ops):
    worst = 0.0
    for n in C.SIZES:
        case = C.make('exact', n)
        src, tgt, init = cuda32(case.src), cuda32(case.ref), near_motion(case)
        one = ops.icp_point_to_point(src, tgt, ICP_RADIUS, init=init, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
        two = ops.icp_point_to_point(src, tgt, ICP_RADIUS, init=init, max_iteration=2, relative_fitness=0.0, relative_rmse=0.0)
        assert (one.iterations, two.iterations) == (1, 2)
        worst = max(worst, float(np.abs(two.transformation - one.transformation).max()))
        assert np.abs(two.transformation - one.transformation).max() <= 1e-12, (n, worst)
        assert C.angle_deg(one.transformation[:3, :3], C.EXACT_TURN) <= 1e-6 and np.abs(one.transformation[:3, 3] - C.EXACT_SHIFT).max() <= 1e-9
    print('icp exact: second iteration moves T by', worst)


# ------------------------------------------------------------------------------------------------------------------ RANSAC
def ransac(ops, case, k, iters, seed, threshold=RANSAC_THRESHOLD):
    T, stats, rmse, hyp = ops.ransac_correspondences(cuda32(case.src), cuda32(case.ref), threshold, k, iters, seed=seed, return_hypotheses=True)
    return T.cpu().numpy(), stats.cpu().numpy(), float(rmse.cpu()[0]), hyp.cpu().numpy()


@pytest.mark.parametrize('n,k', sorted(RANSAC_SEEDS))
def test_ransac_counts_of_every_minimal_sample_on_exact_rows(ops, n, k):
    """Exact rows in general position, 2 000 iterations: a sample of >= 3 distinct rows recovers the motion (count == n), a
    collinear sample (two distinct rows) keeps at least the rows on its line (B with residual 0 on them), a one-row sample
    counts what the host recounts under (I, r_c - s_c) -- criterion D.  The winner is a best iteration, T meets A and C."""
    from oracle import preprocess
    case = ransac_sets()[n]
    seed = RANSAC_SEEDS[(n, k)]
    T, stats, rmse, hyp = ransac(ops, case, k, RANSAC_ITERATIONS, seed)
    draws = preprocess.ransac_draws(n, k, RANSAC_ITERATIONS, seed)
    seen = {'fit': 0, 'line': 0, 'point': 0}
    for it, d in enumerate(draws):
        cls = C.sample_class(d, case.src)
        seen[cls] += 1
        if cls == 'fit':
            assert hyp[it] == n, (it, d, hyp[it])
        elif cls == 'line':
            assert C.rows_on_line(d, case.src) <= hyp[it] <= n, (it, d, hyp[it])
        else:
            t = case.ref[d[0]].astype(np.float64) - case.src[d[0]].astype(np.float64)
            assert hyp[it] == C.recount(np.eye(3), t, case.src, case.ref, RANSAC_THRESHOLD)[0], (it, d, hyp[it])
    print(f'ransac n {n} ransac_n {k}: samples {seen}, winner {stats}, rmse {rmse}')
    assert stats[1] == n == hyp.max() and hyp[stats[0]] == n and rmse <= 1e-6
    m = C.check(T, case.fit('plain'), 'fp32', where=f'ransac {n} {k}')
    assert m['applies'] == 'ABC' and C.angle_deg(T[:3, :3], C.EXACT_TURN) <= 1e-3 and np.abs(T[:3, 3] - C.EXACT_SHIFT).max() <= 1e-5
    again = ransac(ops, case, k, RANSAC_ITERATIONS, seed)
    assert all(np.array_equal(a, b) for a, b in zip((T, stats, np.float64(rmse), hyp), (again[0], again[1], np.float64(again[2]), again[3])))


@pytest.mark.parametrize('family', ['exact_collinear', 'exact_one_point', 'collinear', 'one_point'])
def test_ransac_on_sets_without_a_unique_fit(ops, family):
    """Every correspondence on one line, or equal: every sample is degenerate.  A one-row sample counts what the host recounts
    under (I, r_c - s_c); a sample of two or more distinct rows fits the whole line (count == n: B leaves residual 0 on it)."""
    from oracle import preprocess
    n, k, iters, seed = 8, 3, 500, 21
    case = C.make(family, n)
    T, stats, rmse, hyp = ransac(ops, case, k, iters, seed)
    draws = preprocess.ransac_draws(n, k, iters, seed)
    seen = {'line': 0, 'point': 0}
    for it, d in enumerate(draws):
        cls = 'point' if family.endswith('one_point') or len(set(d.tolist())) == 1 else 'line'  # (distinct rows are distinct points)
        seen[cls] += 1
        if cls == 'point':
            t = case.ref[d[0]].astype(np.float64) - case.src[d[0]].astype(np.float64)
            want, margin = C.recount(np.eye(3), t, case.src, case.ref, RANSAC_THRESHOLD)
            assert margin > 1e-6 and hyp[it] == want, (it, d, hyp[it], want)
        else:
            assert hyp[it] == n, (it, d, hyp[it])
    print(f'ransac {family}: samples {seen}, winner {stats}, rmse {rmse}')
    assert seen['point'] >= 5 and ('collinear' not in family or seen['line'] >= 20)
    assert stats[1] == hyp.max() == n and hyp[stats[0]] == n
    C.check(T, case.fit('plain'), 'fp32', where=family)


def test_ransac_winner_follows_the_documented_order(ops):
    """Noisy rows (1 cm), threshold 5 cm: many iterations tie in the count and differ in RMSE by far more than round-off.
    stats and rmse are those of the float64 restatement's best iteration: more inliers, then lower RMSE, then lower index."""
    from oracle import preprocess
    case = C.make('noisy', 65)
    k, iters, seed, thr = 4, 2000, 5, 0.05
    T, stats, rmse, hyp = ransac(ops, case, k, iters, seed, thr)
    wT, best, count, wrmse, counts = preprocess.ransac_correspondences(case.src, case.ref, thr, k, iters, seed)
    draws = preprocess.ransac_draws(case.n, k, iters, seed)
    top = np.flatnonzero(hyp == hyp.max())
    assert all(C.sample_class(draws[it], case.src) == 'fit' for it in top), 'a degenerate sample ties for the best count: choose another seed'
    assert len(np.flatnonzero(counts == count)) > 1 and np.array_equal(np.flatnonzero(counts == count), top)
    print(f'ransac noisy: winner {stats} restated ({best}, {count}), rmse {rmse} restated {wrmse}, {len(top)} iterations tie in the count')
    assert (stats[0], stats[1]) == (best, count) and abs(rmse - wrmse) <= 1e-6 * wrmse
    assert C.measure(T, case.fit('plain'), 'fp32')['ortho'] <= 1e-6
    assert C.angle_deg(T[:3, :3], wT[:3, :3]) <= 1e-3 and np.abs(T[:3, 3] - wT[:3, 3]).max() <= 1e-5


# --------------------------------------------------------------------------------------------------------------------- LGR
LGR_SIDE, LGR_RADIUS, LGR_MIN_CORR = 128, 0.6, 3


def run_lgr(ops, src, ref, steps):
    """One patch with the correspondences planted on the diagonal of log_scores (score e^0, -60 elsewhere), masks over the
    first n rows -> (ref rows, src rows, scores, T, counts) as numpy."""
    n = len(src)
    L = np.full((1, LGR_SIDE + 1, LGR_SIDE + 1), -60.0, np.float32)
    L[0, np.arange(n), np.arange(n)] = 0.0
    rp, sp = np.zeros((1, LGR_SIDE, 3), np.float32), np.zeros((1, LGR_SIDE, 3), np.float32)
    rp[0, :n], sp[0, :n] = ref, src
    mask = np.zeros((1, LGR_SIDE), np.uint8)
    mask[0, :n] = 1
    rc, sc, cs, T, counts = ops.lgr(torch.from_numpy(L).cuda(), torch.from_numpy(rp).cuda(), torch.from_numpy(sp).cuda(),
                                    torch.from_numpy(mask).cuda(), torch.from_numpy(mask).cuda(), LGR_RADIUS, LGR_MIN_CORR, steps)
    counts = counts.cpu().numpy()
    c = int(counts[0])
    return rc[:c].cpu().numpy(), sc[:c].cpu().numpy(), cs[:c].cpu().numpy(), T.cpu().numpy(), counts


@pytest.mark.parametrize('family', ['full', 'coplanar', 'near_coplanar', 'collinear', 'half_turn', 'mirrored_flat', 'exact', 'exact_collinear'])
def test_lgr_pose_with_and_without_the_carried_basis(ops, family):
    """steps = 1 (no carried basis in the last fit but the identity) and steps = 5 (the eigenvector frame carried over four
    fits of the same covariance): A, B, C against the scored-rule fit of the final inliers, which are all the planted rows; and
    steps = 5 equals steps = 1 within C where the optimum is unique."""
    worst = {}
    for n in (3, 4, 64, 65):
        case = C.make(family, n)
        poses = {}
        for steps in (1, 5):
            rc, sc, cs, T, counts = run_lgr(ops, case.src, case.ref, steps)
            where = f'{case.name} steps {steps}'
            assert np.array_equal(rc, case.ref) and np.array_equal(sc, case.src) and np.array_equal(cs, np.ones(n, np.float32)), where
            assert counts.tolist() == [n, 1, 0] and np.array_equal(T[3], [0, 0, 0, 1]), where
            inl, edge = lgr_options_restatement.final_inliers(T, rc, sc, LGR_RADIUS)
            assert inl.all() and edge > 1e-4, (where, edge)
            fit = C.Fit(sc, rc, 'scored', cs * inl, family)
            m = C.check(T, fit, 'fp32', where=where, worst=worst)
            assert m['applies'] == ('AB' if 'collinear' in family else 'ABC'), (where, m)
            poses[steps] = T
        if fit.unique:
            d = C.angle_deg(poses[5][:3, :3], poses[1][:3, :3]), float(np.abs(poses[5][:3, 3] - poses[1][:3, 3]).max())
            worst['carried angle'], worst['carried trans'] = max(worst.get('carried angle', 0.0), d[0]), max(worst.get('carried trans', 0.0), d[1])
            assert d[0] <= 1e-3 and d[1] <= 1e-5, (case.name, d)
    report(f'lgr {family}', worst)


@pytest.mark.parametrize('steps', [1, 5])
def test_lgr_refinement_gate_closed_on_every_row_returns_the_identity(ops, steps):
    """Rows that follow no rigid motion: the hypothesis has no inlier, the refinement's covariance is exactly zero and the
    pose is the identity (the guard of lgr.hip: the carried frame must not leak into the result)."""
    rng = np.random.default_rng(3)
    src, ref = (rng.normal(size=(4, 3)) * 100).astype(np.float32), (rng.normal(size=(4, 3)) * 100).astype(np.float32)
    rc, sc, cs, T, counts = run_lgr(ops, src, ref, steps)
    assert len(cs) == 4 and counts.tolist() == [4, 1, 0]
    local = C.Fit(src, ref, 'scored', np.ones(4, np.float32)).transform
    assert not lgr_options_restatement.final_inliers(np.concatenate([local, [[0, 0, 0, 1]]]), ref, src, LGR_RADIUS)[0].any()
    assert np.array_equal(T, np.eye(4, dtype=np.float32)), T


# ------------------------------------------------------------------------------------------------------------------ robust
@pytest.mark.parametrize('family', ['exact', 'exact_coplanar', 'exact_collinear'])
def test_robust_registration_on_all_inlier_exact_sets(ops, family):
    """All rows are inliers of one exact motion (noise bound 0.01, the fixtures'): graph, selection, weights and counts equal
    the restatement's; the pose is compared through the module's same_pose where the restatement has a spread under
    reordering (exact data sum without rounding in any order, so mostly it has none, and the fp64 bounds of C against the
    reference take its place); A always, C where the optimum is unique -- the pairwise covariance the estimator solves is K
    times the plain rule's."""
    from test_robust_gpu import run, same_graph, same_pose
    worst = {}
    for n in (3, 4, 65):
        case = C.make(family, n)
        want = RR.robust_registration(case.src, case.ref, 0.01)
        RR.check_fixture(want)
        got = run(ops, case.src, case.ref, 0.01)
        same_graph(got, want, case.name)
        assert got.num_selected == n and got.valid == 1 and got.exact == 1 and got.translation_inliers == n == want.translation_inliers
        assert np.array_equal(got.weights, want.weights) and abs(got.iterations - want.iterations) <= 1
        assert np.array_equal(got.transformation[3], [0, 0, 0, 1])
        fit = case.fit('plain')
        m = C.check(got.transformation, fit, 'fp64', where=case.name, worst=worst)
        assert m['applies'] == ('AB' if family == 'exact_collinear' else 'ABC')
        if fit.unique:
            dR, dt, dw, its = RR.permutation_spread(case.src, case.ref, want, noise_bound=0.01)
            print(case.name, 'restatement spread', dR, dt)
            if dR > 0 and dt > 0:
                same_pose(got, want, case.src, case.ref, 0.01, case.name)
            assert C.angle_deg(got.transformation[:3, :3], want.transform[:3, :3]) <= 1e-6
            assert np.abs(got.transformation[:3, 3] - want.transform[:3, 3]).max() <= 1e-9
    report(f'robust {family}', worst)
