"""Marginal covariances of the pose graph on the host: the kernels' work-item functions compiled for the host
(rdm_pose_graph_marginals_host) against the long-double inverse of tests/pose_graph_marginals_restatement.py, the refusals and
ops.pose_graph_marginals' argument checks.  No GPU.  The accuracy criterion is the restatement's: the largest per-block relative
error <= max(10 x np.linalg.inv's on the same matrix, 1e-14); every test prints the ratio."""
import ctypes

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_marginals_restatement as M
from test_pose_graph_direct import dense, random_system, separator


def lib():
    from rdmnet_amd import _lib
    return _lib.lib()


def marginals_host(n, edges, diag, off, fill=np.nan):
    edges = np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)
    diag, off = (np.ascontiguousarray(a, dtype=np.float64) for a in (diag, off))
    out = np.full((n, 6, 6), fill)
    rc = lib().rdm_pose_graph_marginals_host(n, len(edges), edges.ctypes.data, diag.ctypes.data, off.ctypes.data, out.ctypes.data)
    return rc, out


def system(c, weights):
    """The library's own per-edge blocks at the case's poses (unit weight), times the weights, summed as the kernels' assembly sums
    them: diag [n, 36] and off [E, 36] of rdm_pose_graph_marginals_host."""
    n, E = len(c['nodes']), len(c['edges'])
    out = np.zeros((E, 128))
    diag = np.zeros((n, 36))
    for e, (s, t) in enumerate(c['edges'].tolist()):
        Xs, Xt, T, L = (np.ascontiguousarray(a, dtype=np.float64) for a in (c['nodes'][s], c['nodes'][t], c['transforms'][e],
                                                                             c['informations'][e]))
        assert lib().rdm_pose_graph_edge_terms_host(Xs.ctypes.data, Xt.ctypes.data, T.ctypes.data, L.ctypes.data, ctypes.c_double(0.0), 0,
                                                    out[e].ctypes.data) == 0
        diag[s] += weights[e] * out[e, 8:44]
        diag[t] += weights[e] * out[e, 80:116]
    return diag, weights[:, None] * out[:, 44:80]


# ---- 1. accuracy on the pose graphs -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(M.GRAPHS))
def test_host_marginals_match_the_long_double_inverse(name):
    c, w, ref = M.graph(name)
    n = len(c['nodes'])
    diag, off = system(c, w)
    A = dense(n, c['edges'], diag, off)
    assert np.abs(A - ref.A).max() <= 1e-12 * np.abs(ref.A).max()  # the library's blocks are the restatement's H
    rc, cov = marginals_host(n, c['edges'], diag, off)
    assert rc == 0
    print('separator', separator(n, c['edges'])[0], 'condition %.1e' % np.linalg.cond(ref.A))
    ref.check(name, cov)
    again = marginals_host(n, c['edges'], diag, off)[1]
    assert np.array_equal(cov, again)


def test_closed_form_one_edge_at_zero_residual():
    c, L = M.closed_form()
    diag, off = system(c, np.ones(1))
    rc, cov = marginals_host(2, c['edges'], diag, off)
    assert rc == 0
    M.Reference(0.5 * (L + L.T)).check('closed form', cov)  # Sigma_1 = L^-1: the factor is H^-1 and the tangent is rotation first


# ---- 2. the smallest shapes at which the elimination can go wrong -------------------------------------------------------------------

# name -> (nodes, chords, the separator the rule gives)
SHAPES = {
    'one free node': (2, [], []),
    'chain of three': (3, [], []),
    'separator at node 1, the run starts behind it': (5, [(1, 3)], [1]),
    'separator at the last node': (8, [(7, 2), (7, 4)], [7]),
    'adjacent separators': (14, [(3, 6), (3, 8), (4, 10), (4, 12)], [3, 4]),
    'run of one node': (12, [(3, 7), (3, 9), (5, 1), (5, 11)], [3, 5]),
    'chord into the middle of a run': (12, [(11, 5), (11, 7)], [11]),
    'two couplings that begin at different positions': (14, [(3, 6), (3, 8), (12, 7), (12, 9)], [3, 12]),
    # (every pair of the four free nodes is joined; the rule covers the three off-chain pairs with nodes 1 and 2, the runs are {3, 4})
    'K4 on nodes 1 to 4': (5, [(1, 3), (1, 4), (2, 4)], [1, 2]),
    'far node with an edge to node 0': (8, [(7, 0), (2, 5)], [2]),
    'double edge on a chord': (10, [(2, 6), (2, 6)], [2]),
    'double edge between separators': (14, [(3, 6), (3, 8), (10, 5), (10, 12), (3, 10), (3, 10)], [3, 10]),
    'small hub': (8, [(4, 1), (4, 2), (4, 6), (4, 7)], [4]),
    # (twelve disjoint chords, each covered by its lower end: the run 13 .. 45 couples to twelve separator nodes, 72 columns of Psi
    # for the run sweep's 64 lanes)
    'more than 64 columns in a run': (46, [(k, 20 + 2 * k) for k in range(1, 13)], list(range(1, 13))),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_host_marginals_on_the_small_shapes(name):
    n, chords, want = SHAPES[name]
    edges, diag, off, _ = random_system(n, chords, seed=300 + n + len(chords))
    size, out = separator(n, edges)
    assert out[:size].tolist() == want
    rc, cov = marginals_host(n, edges, diag, off)
    assert rc == 0
    M.Reference(dense(n, edges, diag, off)).check(name, cov)


# ---- 3. monotonicity ----------------------------------------------------------------------------------------------------------------

def test_a_further_loop_edge_never_increases_a_marginal():
    c, w, ref = M.graph('noisy')
    n = len(c['nodes'])
    rng = np.random.default_rng(5)
    more = dict(c)
    s, t = 55, 12
    T = cases.inverse(c['nodes'][t]) @ c['nodes'][s]
    T[3] = (0.0, 0.0, 0.0, 1.0)
    more['edges'] = np.concatenate([c['edges'], [[s, t]]])
    more['transforms'] = np.concatenate([c['transforms'], T[None]])
    more['informations'] = np.concatenate([c['informations'], cases.random_information(rng)[None]])
    w2 = np.concatenate([w, [1.0]])
    ref2 = M.Reference(M.information(more['nodes'], more['edges'], more['transforms'], more['informations'], w2)[6:, 6:])
    cov = marginals_host(n, c['edges'], *system(c, w))[1]
    cov2 = marginals_host(n, more['edges'], *system(more, w2))[1]
    ref2.check('noisy plus a loop', cov2)
    worst = 0.0
    for i in range(1, n):
        # the exact difference is negative semi-definite; each block is within bound * max|block| per entry, a 6 x 6 perturbation
        # moves an eigenvalue by at most 6 times its largest entry
        slack = 6.0 * (ref.bound * np.abs(ref.blocks[i - 1]).max() + ref2.bound * np.abs(ref2.blocks[i - 1]).max())
        top = np.linalg.eigvalsh(cov2[i] - cov[i])[-1]
        worst = max(worst, top / slack)
        assert top <= slack, f'node {i}: the marginal grew by {top:.3e} (slack {slack:.3e})'
    shrink = min(np.trace(cov2[i]) / np.trace(cov[i]) for i in range(1, n))
    print(f'largest growth / slack {worst:.2e}; the trace of the most improved node falls to {shrink:.3f} of its value')
    assert shrink < 1.0


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def over_the_cap():
    """A chain of 601 nodes with 300 disjoint chords (i, i + 2): every chord needs a separator node of its own."""
    chords = [(i, i + 2) for i in range(1, 599) if i % 4 in (1, 2)]
    assert len(chords) == 300 and len({v for ch in chords for v in ch}) == 600
    n = 601
    return n, np.array([(i + 1, i) for i in range(n - 1)] + chords, np.int64)


def test_a_graph_over_the_separator_cap_is_refused_with_the_output_untouched():
    L = lib()
    cap = L.rdm_pose_graph_direct_max_separator()
    assert cap == 256
    n, edges = over_the_cap()
    assert separator(n, edges)[0] == 300
    noff, eoff = np.array([0, n], np.int64), np.array([0, len(edges)], np.int64)
    assert L.rdm_pose_graph_marginals_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data) == 0
    msg = L.rdm_last_error().decode()
    print(msg)
    assert '300' in msg and '256' in msg and 'graph 0' in msg and 'conjugate' not in msg
    # the call itself refuses before any GPU work (no pointer is followed): the covariances and the report stay as they were
    dummy = np.zeros(64)
    cov, report = np.full((n, 36), -7.0), np.full((1, 2), -7.0)
    rc = L.rdm_pose_graph_marginals(1, noff.ctypes.data, eoff.ctypes.data, dummy.ctypes.data, edges.ctypes.data, dummy.ctypes.data,
                                    dummy.ctypes.data, 0, cov.ctypes.data, report.ctypes.data, 0, 0, 0)
    msg = L.rdm_last_error().decode()
    assert rc == -1 and '300' in msg and '256' in msg and 'graph 0' in msg
    assert np.all(cov == -7.0) and np.all(report == -7.0)
    # the host twin likewise
    rng = np.random.default_rng(0)
    diag = np.tile((50.0 * np.eye(6)).reshape(36), (n, 1))
    off = rng.normal(size=(len(edges), 36))
    rc, out = marginals_host(n, edges, diag, off, fill=-7.0)
    msg = L.rdm_last_error().decode()
    assert rc == -1 and '300' in msg and '256' in msg and np.all(out == -7.0)
    # with 256 of the chords the graph fits, and the workspace holds C and Z
    fits = np.ascontiguousarray(edges[:n - 1 + cap])
    eoff[1] = len(fits)
    assert separator(n, fits)[0] == cap
    assert L.rdm_pose_graph_marginals_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, fits.ctypes.data) > 36 * 8 * 2 * cap * cap


def test_pivots_that_are_not_positive_are_refused():
    n, chords, _ = SHAPES['double edge between separators']
    edges, diag, off, _ = random_system(n, chords, seed=77)
    assert marginals_host(n, edges, diag, off)[0] == 0
    bad = diag.copy()
    bad[6] = -bad[6]  # inside a run
    rc, out = marginals_host(n, edges, bad, off, fill=-7.0)
    assert rc == -1 and 'not positive' in lib().rdm_last_error().decode() and np.all(out == -7.0)
    weak = diag.copy()
    weak[10] = 1e-6 * np.eye(6).reshape(36)  # a separator node: positive by itself, indefinite once Y^T Y is taken away
    rc, out = marginals_host(n, edges, weak, off, fill=-7.0)
    assert rc == -1 and 'Schur' in lib().rdm_last_error().decode() and np.all(out == -7.0)


def test_bad_edges_are_refused_by_the_workspace_size():
    L = lib()
    noff, eoff = np.array([0, 5], np.int64), np.array([0, 2], np.int64)
    for edges, word in (([(1, 0), (2, 2)], 'itself'), ([(1, 0), (2, 5)], 'outside')):
        ed = np.array(edges, np.int64)
        assert L.rdm_pose_graph_marginals_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data) == 0
        assert word in L.rdm_last_error().decode()


# ---- 5. the Python layer's checks, before any library call ----------------------------------------------------------------------------

def test_argument_errors_are_value_errors_before_any_library_call(monkeypatch):
    from rdmnet_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was called')

    monkeypatch.setattr(_lib, 'lib', no_library)
    c = cases.consistent('ring3')
    args = (c['nodes'], c['edges'], c['transforms'], c['informations'])
    with pytest.raises(ValueError, match='nodes must be'):
        ops.pose_graph_marginals(c['nodes'][:, :3], *args[1:])
    with pytest.raises(ValueError, match='informations must be'):
        ops.pose_graph_marginals(*args[:3], c['informations'][:, :5])
    with pytest.raises(ValueError, match='one row per edge'):
        ops.pose_graph_marginals(*args[:2], c['transforms'][:2], c['informations'])
    with pytest.raises(ValueError, match='one entry per edge'):
        ops.pose_graph_marginals(*args, np.ones(2))
    with pytest.raises(ValueError, match='weights must be'):
        ops.pose_graph_marginals(*args, np.ones((3, 1)))
    with pytest.raises(ValueError, match='finite and >= 0'):
        ops.pose_graph_marginals(*args, np.array([1.0, -1e-3, 1.0]))
    with pytest.raises(ValueError, match='finite and >= 0'):
        ops.pose_graph_marginals(*args, np.array([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError, match='go together'):
        ops.pose_graph_marginals(*args, graph_node_offsets=[0, 3])
    with pytest.raises(ValueError, match='offsets must be'):
        ops.pose_graph_marginals(*args, graph_node_offsets=[0, 2], graph_edge_offsets=[0, 3])
    with pytest.raises(ValueError, match='pose_graph_marginals: no path of edges connects node 2'):
        ops.pose_graph_marginals(c['nodes'], c['edges'][:1], c['transforms'][:1], c['informations'][:1])


def test_pose_graph_optimize_goes_through_the_same_preparation_with_its_own_name():
    from rdmnet_amd import ops
    c = cases.consistent('ring3')
    with pytest.raises(ValueError, match=r'pose_graph_optimize: nodes must be \[\*, 4, 4\], got \(3, 3, 4\)'):
        ops.pose_graph_optimize(c['nodes'][:, :3], c['edges'], c['transforms'], c['informations'])
    with pytest.raises(ValueError, match='pose_graph_optimize: no path of edges connects node 2 of graph 0 to its node 0'):
        ops.pose_graph_optimize(c['nodes'], c['edges'][:1], c['transforms'][:1], c['informations'][:1])


def test_command_line_offers_the_covariance():
    from rdmnet_amd import trajectory
    ap = trajectory.make_parser()
    assert ap.parse_args(['--features-root', 'x']).covariance is False
    assert ap.parse_args(['--features-root', 'x', '--optimize', '--covariance']).covariance is True
