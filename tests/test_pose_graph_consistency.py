"""Cross covariances and loop-edge consistency of the pose graph on the host: the pairs' work-item functions
compiled for the host (rdm_pose_graph_pair_covariances_host, rdm_pose_graph_pair_terms_host) against the long-double inverse of
tests/pose_graph_consistency_restatement.py under its criteria (numpy is the yardstick; every test prints the ratios), the refusals
and ops.pose_graph_consistency's argument checks.  No GPU."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_consistency_restatement as C
import pose_graph_marginals_restatement as M
import pose_graph_restatement as R
from test_pose_graph_direct import dense, random_system, separator
from test_pose_graph_marginals import SHAPES, marginals_host, system

TERMS = 300  # M and d2 are held on at most about this many of a graph's pairs, evenly strided (each costs three long-double inverses)


def lib():
    from rdmnet_amd import _lib
    return _lib.lib()


def cross_host(n, edges, diag, off, pairs, fill=np.nan):
    edges = np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    diag, off = (np.ascontiguousarray(a, dtype=np.float64) for a in (diag, off))
    out = np.full((len(pairs), 6, 6), fill)
    rc = lib().rdm_pose_graph_pair_covariances_host(n, len(edges), edges.ctypes.data, diag.ctypes.data, off.ctypes.data, len(pairs),
                                                    pairs.ctypes.data, out.ctypes.data)
    return rc, out


def terms_host(Xs, Xt, T, L, Sss, Stt, Sst):
    """-> (return code, r [6], M [6, 6], d2, status)."""
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (Xs, Xt, T)]
    b = [np.ascontiguousarray(x, dtype=np.float64) for x in (Sss, Stt, Sst)]
    Lc = None if L is None else np.ascontiguousarray(L, dtype=np.float64)
    out = np.full(44, -7.0)
    rc = lib().rdm_pose_graph_pair_terms_host(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 0 if Lc is None else Lc.ctypes.data,
                                              b[0].ctypes.data, b[1].ctypes.data, b[2].ctypes.data, out.ctypes.data)
    return rc, out[:6], out[6:42].reshape(6, 6), out[42], int(out[43]) if rc == 0 else -1


def all_pairs(n):
    return np.array([(s, t) for s in range(n) for t in range(n) if s != t], np.int64).reshape(-1, 2)


# ---- 1. every placement of the two nodes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(SHAPES))
def test_all_ordered_pairs_on_the_small_shapes(name):
    """Between them the shapes put the two nodes: both in S; S and a run on either side; the same run with s before and behind t;
    different runs; a run of one node; a coupling that begins behind the row position; node 0 on either side; the 72-column run."""
    n, chords, want = SHAPES[name]
    edges, diag, off, _ = random_system(n, chords, seed=300 + n + len(chords))
    size, out = separator(n, edges)
    assert out[:size].tolist() == want  # the coverage is real
    pairs = all_pairs(n)
    rc, cross = cross_host(n, edges, diag, off, pairs)
    assert rc == 0
    ref = C.Reference(dense(n, edges, diag, off))
    ref.check_cross(name, pairs, cross)
    # Sigma_st against Sigma_ts computed as its own pair: equal transposed within the criterion (bit equality is not required)
    index = {tuple(p): k for k, p in enumerate(pairs.tolist())}
    mirrored = np.stack([cross[index[(t, s)]].T for s, t in pairs.tolist()])
    ref.check_cross(name + ' (transposed)', pairs, mirrored)


# ---- 2. the pose graphs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(M.GRAPHS))
def test_host_pairs_match_the_long_double_inverse(name):
    c, w, ref, pairs, T, L = C.graph(name)
    n = len(c['nodes'])
    diag, off = system(c, w)
    rc, cross = cross_host(n, c['edges'], diag, off, pairs)
    assert rc == 0
    ref.check_cross(name, pairs, cross)
    rc, cov = marginals_host(n, c['edges'], diag, off)
    assert rc == 0
    sub = np.arange(0, len(pairs), max(1, len(pairs) // TERMS))
    got_m, got_d2 = [], []
    for k in sub:
        s, t = pairs[k]
        rc, r, Mk, d2, status = terms_host(c['nodes'][s], c['nodes'][t], T[k], L[k], cov[s], cov[t], cross[k])
        assert rc == 0 and status == 0
        assert np.abs(r - R.residual(c['nodes'][s], c['nodes'][t], T[k])).max() <= 1e-12
        got_m.append(Mk)
        got_d2.append(d2)
    ref.check_terms(name, c['nodes'], pairs[sub], T[sub], L[sub], got_m, got_d2)


def test_a_pair_s_bits_do_not_depend_on_the_other_pairs_or_their_order():
    c, w, ref, pairs, T, L = C.graph('noisy')
    n = len(c['nodes'])
    diag, off = system(c, w)
    whole = cross_host(n, c['edges'], diag, off, pairs)[1]
    assert np.array_equal(whole, cross_host(n, c['edges'], diag, off, pairs)[1])
    rng = np.random.default_rng(3)
    order = rng.permutation(len(pairs))
    assert np.array_equal(cross_host(n, c['edges'], diag, off, pairs[order])[1], whole[order])
    for k in (0, 7, len(pairs) - 1):
        assert np.array_equal(cross_host(n, c['edges'], diag, off, pairs[k:k + 1])[1][0], whole[k])
    # more column nodes than are in flight at a time (128): the chunks do not show
    n = 140
    edges, diag, off, _ = random_system(n, [(5, 60), (5, 100), (30, 120), (131, 70)], seed=11)
    many = np.array([(s, t) for t in range(1, n) for s in (((t + 17) % (n - 1)) + 1, ((t + 50) % (n - 1)) + 1)], np.int64)
    assert len(set(many[:, 1].tolist())) == 139
    rc, whole = cross_host(n, edges, diag, off, many)
    assert rc == 0 and np.all(np.isfinite(whole))
    pick = np.concatenate([[0, 1, 254, 255, 256, 257, len(many) - 1], rng.permutation(len(many))[:20]])
    assert np.array_equal(cross_host(n, edges, diag, off, many[pick])[1], whole[pick])
    for k in (0, 255, 256, len(many) - 1):
        assert np.array_equal(cross_host(n, edges, diag, off, many[k:k + 1])[1][0], whole[k])


# ---- 3. closed form and status --------------------------------------------------------------------------------------------------------

def closed_form_pair():
    c, L = M.closed_form()
    rng = np.random.default_rng(43)
    xi = cases.perturbation(rng, 0.05, 0.3)
    return c, L, R.retract(c['transforms'][0], xi), cases.random_information(rng)


def test_closed_form_candidate_beside_one_edge():
    """One edge (1 -> 0) at zero residual with information L: Sigma_11 = L^-1; the candidate pair (1, 0) with transform T Exp(xi)
    and information L2 has M = L^-1 at T (A = I there) and d2 = r^T (M + L2^-1)^-1 r."""
    c, L, T2, L2 = closed_form_pair()
    diag, off = system(c, np.ones(1))
    rc, cov = marginals_host(2, c['edges'], diag, off)
    rc2, cross = cross_host(2, c['edges'], diag, off, [(1, 0)])
    assert rc == 0 and rc2 == 0 and np.all(cross == 0.0)
    Linv = np.linalg.inv(L)
    rc, r, Mk, d2, status = terms_host(c['nodes'][1], c['nodes'][0], c['transforms'][0], L2, cov[1], cov[0], cross[0])
    assert rc == 0 and status == 0 and np.abs(r).max() <= 1e-12
    assert np.abs(Mk - Linv).max() <= 1e-12 * np.abs(Linv).max() and np.array_equal(Mk, Mk.T)
    rc, r, Mk, d2, status = terms_host(c['nodes'][1], c['nodes'][0], T2, L2, cov[1], cov[0], cross[0])
    want_r, A, _ = R.jacobians(c['nodes'][1], c['nodes'][0], T2)
    want_M = A @ Linv @ A.T
    want = want_r @ np.linalg.solve(want_M + np.linalg.inv(L2), want_r)
    print(f'closed form: d2 {d2:.6g} want {want:.6g}')
    assert rc == 0 and status == 0 and np.abs(r - want_r).max() <= 1e-12
    assert np.abs(Mk - want_M).max() <= 1e-12 * np.abs(want_M).max()
    assert abs(d2 - want) <= 1e-11 * want
    rc, _, _, d2_alone, status = terms_host(c['nodes'][1], c['nodes'][0], T2, None, cov[1], cov[0], cross[0])
    assert rc == 0 and status == 0 and abs(d2_alone - want_r @ np.linalg.solve(want_M, want_r)) <= 1e-11 * d2_alone and d2_alone > d2


def test_an_indefinite_information_is_pair_status_1_with_d2_nan():
    c, L, T2, L2 = closed_form_pair()
    diag, off = system(c, np.ones(1))
    cov = marginals_host(2, c['edges'], diag, off)[1]
    bad = L2.copy()
    bad[2, 2] = -bad[2, 2]
    rc, r, Mk, d2, status = terms_host(c['nodes'][1], c['nodes'][0], T2, bad, cov[1], cov[0], np.zeros((6, 6)))
    assert rc == 0 and status == 1 and np.isnan(d2)
    assert np.all(np.isfinite(Mk)) and np.all(np.isfinite(r))  # the blocks are still written
    turned = T2.copy()
    turned[:3, :3] = turned[:3, :3] @ R.so3_exp(np.array([0.0, 0.0, np.pi]))
    rc = terms_host(c['nodes'][1], c['nodes'][0], turned, L2, cov[1], cov[0], np.zeros((6, 6)))[0]
    assert rc == -1 and 'beyond the supported angle' in lib().rdm_last_error().decode()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def test_bad_pairs_are_refused_with_the_outputs_untouched():
    L = lib()
    n, chords, _ = SHAPES['run of one node']
    edges, diag, off, _ = random_system(n, chords, seed=5)
    noff, eoff = np.array([0, n], np.int64), np.array([0, len(edges)], np.int64)
    good = np.array([(1, 2), (5, 3), (0, 4)], np.int64)
    poff = np.array([0, 3], np.int64)
    assert L.rdm_pose_graph_consistency_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data, poff.ctypes.data,
                                                        good.ctypes.data) > 0
    dummy = np.zeros(64)
    for pairs, words in (([(1, 2), (4, 4), (3, 3)], ('pair 1', 'itself')), ([(1, 2), (2, 1), (3, n)], ('pair 2', 'outside')),
                         ([(-1, 2), (2, 1), (3, 1)], ('pair 0', 'outside'))):
        pr = np.array(pairs, np.int64)
        assert L.rdm_pose_graph_consistency_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data, poff.ctypes.data,
                                                            pr.ctypes.data) == 0
        msg = L.rdm_last_error().decode()
        assert all(w in msg for w in words), msg
        # the call refuses before any GPU work (no device pointer is followed)
        outs = [np.full(k, -7.0) for k in (36 * n, 108, 108, 3, 2)]
        status = np.full(3, 9, np.uint8)
        rc = L.rdm_pose_graph_consistency(1, noff.ctypes.data, eoff.ctypes.data, dummy.ctypes.data, edges.ctypes.data, dummy.ctypes.data,
                                          dummy.ctypes.data, 0, poff.ctypes.data, pr.ctypes.data, dummy.ctypes.data, 0, outs[0].ctypes.data,
                                          outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data, status.ctypes.data,
                                          outs[4].ctypes.data, 0, 0, 0)
        msg = L.rdm_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), msg
        assert all(np.all(o == -7.0) for o in outs) and np.all(status == 9)
        rc, out = cross_host(n, edges, diag, off, pr, fill=-7.0)
        assert rc == -1 and all(w in L.rdm_last_error().decode() for w in words) and np.all(out == -7.0)
    # what the marginals call refuses comes first: an edge outside its graph, pair offsets that do not fit
    broken = edges.copy()
    broken[3] = (2, n)
    assert L.rdm_pose_graph_consistency_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, broken.ctypes.data, poff.ctypes.data,
                                                        np.array([(4, 4)] * 3, np.int64).ctypes.data) == 0
    assert 'edge 3' in L.rdm_last_error().decode()
    down = np.array([2, 0], np.int64)
    assert L.rdm_pose_graph_consistency_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data, down.ctypes.data,
                                                        good.ctypes.data) == 0
    assert 'pair offsets' in L.rdm_last_error().decode()
    # a failed pivot, as the marginals' twin refuses it
    bad = diag.copy()
    bad[6] = -bad[6]
    rc, out = cross_host(n, edges, bad, off, good, fill=-7.0)
    assert rc == -1 and 'not positive' in L.rdm_last_error().decode() and np.all(out == -7.0)


# ---- 5. the Python layer's checks, before any library call ------------------------------------------------------------------------------

def test_argument_errors_are_value_errors_before_any_library_call(monkeypatch):
    from rdmnet_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was called')

    monkeypatch.setattr(_lib, 'lib', no_library)
    c = cases.consistent('ring3')
    args = (c['nodes'], c['edges'], c['transforms'], c['informations'])
    T2, L2 = np.stack([np.eye(4)] * 2), np.stack([np.eye(6)] * 2)
    with pytest.raises(ValueError, match='pose_graph_consistency: nodes must be'):
        ops.pose_graph_consistency(c['nodes'][:, :3], *args[1:], pairs=[(1, 2)])
    with pytest.raises(ValueError, match='pose_graph_consistency: no path of edges connects node 2'):
        ops.pose_graph_consistency(c['nodes'], c['edges'][:1], c['transforms'][:1], c['informations'][:1], pairs=[(1, 2)])
    with pytest.raises(ValueError, match='finite and >= 0'):
        ops.pose_graph_consistency(*args, np.array([1.0, -1.0, 1.0]), pairs=[(1, 2)])
    with pytest.raises(ValueError, match=r'pairs must be integers \[\*, 2\]'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2, 0)])
    with pytest.raises(ValueError, match=r'pairs must be integers \[\*, 2\]'):
        ops.pose_graph_consistency(*args, pairs=np.array([(1.0, 2.0)]))
    with pytest.raises(ValueError, match='pair_transforms must be'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2)], pair_transforms=T2)
    with pytest.raises(ValueError, match='pair_informations must be'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2), (2, 1)], pair_transforms=T2, pair_informations=L2[:, :5])
    with pytest.raises(ValueError, match='pair 1 joins node 2 to itself'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2), (2, 2)])
    with pytest.raises(ValueError, match=r'pair 0 \(1, 3\) is outside its graph of 3 nodes'):
        ops.pose_graph_consistency(*args, pairs=[(1, 3), (2, 1)])
    with pytest.raises(ValueError, match='graph_pair_offsets goes with'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2)], graph_pair_offsets=[0, 1])
    with pytest.raises(ValueError, match='graph_pair_offsets must be'):
        ops.pose_graph_consistency(*args, pairs=[(1, 2)], graph_node_offsets=[0, 3], graph_edge_offsets=[0, 3], graph_pair_offsets=[0, 2])


def test_command_line_offers_the_loop_consistency_and_the_gate(tmp_path):
    from rdmnet_amd import trajectory
    ap = trajectory.make_parser()
    plain = ap.parse_args(['--features-root', 'x'])
    assert plain.loop_consistency is False and plain.loop_gate is None
    assert ap.parse_args(['--features-root', 'x', '--loop-consistency']).loop_consistency is True
    assert ap.parse_args(['--features-root', 'x', '--optimize', '--loop-gate', '25']).loop_gate == 25.0
    with pytest.raises(trajectory.TrajectoryError, match='--loop-gate needs --optimize'):
        trajectory.run(ap.parse_args(['--features-root', str(tmp_path), '--loop-gate', '25']))
