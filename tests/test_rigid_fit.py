"""CPU: the cases of rigid_fit_cases.py hold the edges they were built for, the float64 reference meets its own criteria
(and, rounded to float32, the fp32 bounds the GPU half uses), and the five float64 solvers the suite already carries agree
with it.  Prints the reference's worst figure per family and criterion (DESIGN.md 7 records the table)."""
import numpy as np
import pytest

import eval_restatement
import icp_restatement
import rigid_fit_cases as C
import robust_restatement

RULES = [('plain', None)] + [('scored', p) for p in C.PATTERNS]
RANSAC_SEEDS = {(3, 3): 11, (4, 3): 12, (4, 4): 13, (8, 3): 14, (8, 4): 15}  # (rows, ransac_n) -> seed of the GPU half
RANSAC_ITERATIONS = 2000
RANSAC_THRESHOLD = 0.3


def all_fits():
    """Every (case, rule, scores, fit), built once."""
    if not hasattr(all_fits, 'cache'):
        out = []
        for family in C.FAMILIES:
            for n in C.sizes_of(family):
                case = C.make(family, n)
                for rule, pattern in RULES:
                    scores = None if pattern is None else C.scores_of(pattern, case.n)
                    out.append((case, rule, pattern, scores, case.fit(rule, scores)))
        all_fits.cache = out
    return all_fits.cache


def test_numpy_svd_of_a_zero_matrix_gives_the_identity():
    R, S, d = C.solve(np.zeros((3, 3)))
    assert np.array_equal(R, np.eye(3)) and not S.any() and d == 1.0


def test_every_case_holds_the_edge_it_was_built_for():
    for family in C.FAMILIES:
        for n in C.sizes_of(family):
            case = C.make(family, n)
            f = case.fit('plain')
            assert case.src.dtype == np.float32 and case.src.shape == (case.n, 3) == case.ref.shape
            if family != 'far':
                assert max(np.abs(case.src).max(), np.abs(case.ref).max()) <= 80.0, case.name
            rank = min(C.RANK[family], case.n - 1)
            s = f.S / f.S[0] if f.S[0] > 0 else f.S
            # a missing dimension is left to the float32 rounding of the stored rows (2^-24 of 80 m against 1 m of spread,
            # squared in H), or to the slab thickness of the near-flat families
            small = 1e-5 if family in ('near_coplanar', 'mirrored_flat') else 1e-9
            got = int((s > small).sum()) if f.S[0] > 0 else 0
            assert got == rank, (case.name, f.S, rank)
            if family.endswith('one_point') or family == 'single':
                assert f.zero and not f.unique, case.name  # n equal float32 rows sum and divide exactly in float64
            if family in ('mirrored', 'mirrored_flat', 'mirrored_tie') and s[2] > 1e-9:
                assert f.d == -1.0, case.name
            elif s[2] > 1e-9:
                assert f.d == 1.0, case.name
            if family in ('full', 'noisy', 'coplanar', 'near_coplanar', 'half_turn', 'far', 'exact', 'exact_coplanar', 'mirrored_flat') or \
                    (family == 'mirrored' and case.n >= 4):
                assert f.unique, (case.name, f.gap)
            if family in ('collinear', 'exact_collinear', 'two', 'mirrored_tie'):
                assert not f.unique and not f.zero, (case.name, f.gap)
            if family == 'mirrored_tie':
                assert abs(f.S[1] - f.S[2]) <= 1e-12 * f.S[0] and f.S[1] > 0.1 * f.S[0], f.S
                assert np.array_equal(f.H, f.H.astype(np.float32))  # formed without rounding
            if family == 'half_turn':
                assert np.array_equal(case.motion[:3, :3], np.diag([1.0, -1.0, -1.0]))
                assert abs(np.trace(f.R) + 1.0) < 1e-6  # quaternion w = 0
            if family == 'mirrored_flat':
                assert abs(np.trace(f.R) + 1.0) < 1e-2, np.trace(f.R)  # the proper optimum of an in-plane mirror: a half turn
            if family.startswith('exact') and f.unique:
                assert C.angle_deg(f.R, C.EXACT_TURN) < 1e-12 and np.abs(f.t - C.EXACT_SHIFT).max() < 1e-12
    # the scored patterns: all zero -> H == 0 and T the identity; one negative score counts as 0; sum s = 1e-5 halves the weights
    case = C.make('full', 65)
    z = case.fit('scored', C.scores_of('zero', 65))
    assert z.zero and not z.cs.any() and not z.cr.any() and np.array_equal(z.transform, np.eye(4)[:3])
    neg = C.scores_of('negative', 65)
    assert (neg < 0).sum() == 1 and np.array_equal(case.fit('scored', neg).H, case.fit('scored', np.maximum(neg, 0)).H)
    tiny = C.scores_of('tiny', 65)
    assert abs(tiny.astype(np.float64).sum() / 1e-5 - 1.0) < 1e-6
    assert np.abs(case.fit('scored', tiny).cs / case.src.astype(np.float64).T.dot(tiny / tiny.astype(np.float64).sum()) - 0.5).max() < 1e-6
    one = C.scores_of('one', 65)
    assert (one == 1).sum() == 1 and (one == 0).sum() == 64 and not case.fit('scored', one).unique
    # a tie case away from the origin is a near-tie under the scored rule (the centroids are not renormalised): still not unique
    assert not C.tie_case((16.0, -8.0, 4.0)).fit('scored', np.ones(6, np.float32)).unique


def test_the_reference_meets_its_criteria_in_float64_and_rounded_to_float32():
    """A to D with the fp64 bounds on the reference itself, and with the fp32 bounds on its float32 rounding: the proof that
    the fp32 bounds of the GPU half can be met at all."""
    table = {}
    for case, rule, pattern, scores, f in all_fits():
        T = f.transform
        for out, Tout in (('fp64', T), ('fp32', T.astype(np.float32))):
            w = table.setdefault((case.family, out), {})
            C.check(Tout, f, out, where=f'{case.name} {rule} {pattern} {out}', worst=w)
            if f.unique:
                w['trans_bound'] = max(w.get('trans_bound', 0.0), C.trans_bound(f, out))
    print('\nfamily            out   ortho      trace/s1   angle deg  trans m    (trans bound)')
    for (family, out), w in sorted(table.items(), key=lambda kv: (C.FAMILIES.index(kv[0][0]), kv[0][1])):
        print(f'{family:17s} {out}  ' + '  '.join(f'{w[k]:9.2e}' if k in w else '    -    ' for k in ('ortho', 'trace', 'angle', 'trans', 'trans_bound')))


def _T12(T):
    return np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)


def test_the_suites_float64_solvers_agree_with_the_reference():
    """oracle.forward.procrustes_fp64, eval_restatement.weighted_procrustes, icp_restatement.kabsch,
    robust_restatement.horn_rotation and the SVD inside oracle.preprocess.ransac_correspondences: 1e-9 degrees and 1e-12 m of
    `solve` where the optimum is unique, criterion B (fp64) where it is not.  The translation bound scales with the lever arm
    |c_s| / 80 m of the family `far` (coordinates of 2e4 m)."""
    from oracle import forward as ofw
    from oracle import preprocess
    worst = {}

    def compare(name, T, f, case):
        T = np.asarray(T, np.float64)
        m = C.measure(np.concatenate([T[:3, :3], (T[:3, 3] if T.shape[1] == 4 else f.cr - T[:3, :3] @ f.cs)[:, None]], 1), f, 'fp64')
        w = worst.setdefault(name, {})
        lever = max(1.0, np.abs(f.cs).max() / 80.0)  # t = c_r - R c_s: a difference in R reaches t over |c_s|
        for k in ('trace', 'angle', 'trans'):
            if k in m:
                w[k] = max(w.get(k, 0.0), m[k] / (lever if k == 'trans' else 1.0))
        assert m['trace'] <= 1e-13, (name, case.name, m)
        if f.unique:
            assert m['angle'] <= 1e-9 and m['trans'] <= 1e-12 * lever, (name, case.name, m)

    for case, rule, pattern, scores, f in all_fits():
        if f.zero:
            continue  # (criterion D is the subject of the first test; the restatements guard H == 0 each in its own way)
        compare('horn_rotation', robust_restatement.horn_rotation(f.H), f, case)
        if rule == 'plain':
            compare('kabsch', _T12(icp_restatement.kabsch(case.src.astype(np.float64), case.ref.astype(np.float64))), f, case)
            if case.n >= 3:  # one iteration whose sample holds min(n, 8) distinct rows: the fit of exactly these rows
                k = min(case.n, 8)
                seed = next(s for s in range(100000) if len(set(preprocess.ransac_draws(case.n, k, 1, s)[0].tolist())) == k)
                rows = preprocess.ransac_draws(case.n, k, 1, seed)[0]
                T = preprocess.ransac_correspondences(case.src, case.ref, 1e6, k, 1, seed)[0]
                sub = case.fit('plain', rows=rows)
                if not sub.zero:
                    compare('ransac', T[:3], sub, case)
        else:
            compare('weighted_procrustes', eval_restatement.weighted_procrustes(case.src, case.ref, scores)[:3], f, case)
            if pattern != 'negative':  # (procrustes_fp64 takes weights, already clamped)
                compare('procrustes_fp64', ofw.procrustes_fp64(case.src, case.ref, scores.astype(np.float64))[0][:3], f, case)
    for name, w in worst.items():
        print(name, {k: f'{v:.2e}' for k, v in w.items()})
    assert set(worst) == {'horn_rotation', 'kabsch', 'ransac', 'weighted_procrustes', 'procrustes_fp64'}


def ransac_sets():
    """The RANSAC sets of the GPU half: exact rows in general position (no three on a line) with n in {3, 4, 8}."""
    out = {}
    for n in (3, 4, 8):
        seed = 0
        while True:
            case = C.make('exact', n, seed=500 + seed)
            p = case.src.astype(np.float64)
            if all(np.linalg.matrix_rank(p[[i, j, k]][1:] - p[i]) == 2 for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)):
                break
            seed += 1
        out[n] = case
    return out


def test_ransac_draws_of_the_chosen_seeds_hold_every_sample_class():
    """Each class of minimal sample occurs at least 20 times in the 2 000 draws of every (rows, ransac_n) of the GPU half --
    but the one-row samples of (8, 4), of which 2000 / 512 = 3.9 are expected: at least one there -- and no recounted
    residual of a one-row hypothesis lies within 1e-6 m of the threshold."""
    from oracle import preprocess
    sets = ransac_sets()
    for (n, k), seed in RANSAC_SEEDS.items():
        case = sets[n]
        draws = preprocess.ransac_draws(n, k, RANSAC_ITERATIONS, seed)
        cls = [C.sample_class(d, case.src) for d in draws]
        counts = {c: cls.count(c) for c in ('fit', 'line', 'point')}
        print(f'n {n} ransac_n {k} seed {seed}: {counts}')
        assert counts['fit'] >= 20 and counts['line'] >= 20 and counts['point'] >= (1 if (n, k) == (8, 4) else 20), counts
        for d, c in zip(draws, cls):
            if c == 'point':
                t = case.ref[d[0]].astype(np.float64) - case.src[d[0]].astype(np.float64)
                assert C.recount(np.eye(3), t, case.src, case.ref, RANSAC_THRESHOLD)[1] > 1e-6
            if c == 'line':
                assert C.rows_on_line(d, case.src) == len(set(d.tolist())) == 2
