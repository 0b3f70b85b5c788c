"""The direct sparse solve of the pose-graph optimisation, on the host: the separator rule
(rdm_pose_graph_separator_host), the kernels' factor, border, Schur and solve functions compiled for the host
(rdm_pose_graph_direct_host) against np.linalg.solve, the refusals and the option's argument checks.  No GPU.

The criterion of every solve is the relative residual max|A x - rhs| / max|rhs| <= max(10 r_numpy, 1e-14), r_numpy the residual of
np.linalg.solve on the same dense matrix: numpy is the reference, the factor 10 covers a hand-written block elimination against
LAPACK's pivoted dense solve, the floor covers tiny systems where numpy's residual is a few 1e-17.  The solutions themselves are
not compared: at condition numbers up to 8e13 two backward-stable solvers differ by 2e-7."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS = (1e-6, 1e-12)


def lib():
    from rdmnet_amd import _lib
    return _lib.lib()


def bench_graph():
    spec = importlib.util.spec_from_file_location('pose_graph_bench', os.path.join(ROOT, 'tools', 'pose_graph_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.graph(500, 40, 0)


# name -> (case, mu of the line process, separator size under the rule)
GRAPHS = {
    'pair': (lambda: cases.consistent('pair'), None, 0),
    'ring3': (lambda: cases.consistent('ring3'), None, 0),
    'double': (lambda: cases.consistent('double'), None, 0),
    'tree': (lambda: cases.tree(), None, 0),
    'ring40': (lambda: cases.consistent('ring40'), None, 3),
    'hub': (lambda: cases.consistent('hub'), None, 1),
    'noisy': (lambda: cases.noisy(), 1.0, 8),
    'gross': (lambda: cases.noisy(gross=3), 1.0, 8),
    'big': (lambda: cases.consistent('big'), None, 103),
    'bench': (bench_graph, 1.0, 38),
}
_cache = {}


def graph(name):
    if name not in _cache:
        _cache[name] = GRAPHS[name][0]()
    return _cache[name]


def separator(n, edges, capacity=None):
    edges = np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)
    cap = n if capacity is None else capacity
    out = np.full(max(cap, 1) + 4, -7, np.int64)
    size = lib().rdm_pose_graph_separator_host(n, len(edges), edges.ctypes.data, out.ctypes.data, cap)
    return size, out


def off_chain_pairs(edges):
    return {(min(s, t), max(s, t)) for s, t in np.asarray(edges).tolist() if s != 0 and t != 0 and abs(s - t) > 1}


# ---- 1. the separator ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(GRAPHS))
def test_separator_covers_the_off_chain_edges(name):
    c, want = graph(name), GRAPHS[name][2]
    n, edges = len(c['nodes']), c['edges']
    size, out = separator(n, edges)
    S = out[:size].tolist()
    print(name, 'nodes', n, 'edges', len(edges), 'separator', size, S[:12])
    assert size == want
    assert S == sorted(set(S)) and 0 not in S and all(0 < v < n for v in S)
    assert np.all(out[size:] == -7)
    assert all(s in S or t in S for s, t in off_chain_pairs(edges))
    if name == 'hub':
        assert S == [7]
    again, out2 = separator(n, edges)
    assert again == size and np.array_equal(out, out2)
    perm = np.random.default_rng(3).permutation(len(edges))
    shuffled, out3 = separator(n, edges[perm])
    assert shuffled == size and np.array_equal(out, out3)
    if size > 1:  # a capacity below |S|: the size all the same, and only `capacity` entries written
        short, out4 = separator(n, edges, capacity=size - 1)
        assert short == size and out4[:size - 1].tolist() == S[:size - 1] and np.all(out4[size - 1:] == -7)


def test_separator_refuses_bad_edges():
    assert separator(5, [(1, 0), (2, 2)])[0] == -1
    assert separator(5, [(1, 0), (2, 5)])[0] == -1
    assert separator(5, [(1, 0), (-1, 3)])[0] == -1
    assert separator(5, [(1, 0), (2, 1), (4, 2)])[0] == 1


# ---- 2. the solve against numpy -------------------------------------------------------------------------------------------------

def direct_host(n, edges, diag, off, rhs):
    edges = np.ascontiguousarray(edges, dtype=np.int64).reshape(-1, 2)
    diag, off, rhs = (np.ascontiguousarray(a, dtype=np.float64) for a in (diag, off, rhs))
    out = np.full((n, 6), np.nan)
    rc = lib().rdm_pose_graph_direct_host(n, len(edges), edges.ctypes.data, diag.ctypes.data, off.ctypes.data, rhs.ctypes.data,
                                          out.ctypes.data)
    return rc, out


def dense(n, edges, diag, off):
    """The arrays rdm_pose_graph_direct_host takes, as a dense matrix over the free nodes 1 .. n - 1."""
    A = np.zeros((6 * n, 6 * n))
    for i in range(n):
        d = diag[i].reshape(6, 6)
        A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.tril(d) + np.tril(d, -1).T
    for e, (s, t) in enumerate(np.asarray(edges).reshape(-1, 2).tolist()):
        A[6 * s:6 * s + 6, 6 * t:6 * t + 6] += off[e].reshape(6, 6)
        A[6 * t:6 * t + 6, 6 * s:6 * s + 6] += off[e].reshape(6, 6).T
    return A[6:, 6:]


def residuals(n, edges, diag, off, rhs):
    """-> (return code, the direct solve's relative residual, numpy's, the dense matrix)."""
    A = dense(n, edges, diag, off)
    b = np.asarray(rhs).reshape(-1)[6:]
    rc, x = direct_host(n, edges, diag, off, rhs)
    if rc != 0:
        return rc, np.inf, np.inf, A
    assert np.all(x[0] == 0.0) and np.all(np.isfinite(x))
    scale = np.abs(b).max()
    r_direct = np.abs(A @ x.reshape(-1)[6:] - b).max() / scale
    r_numpy = np.abs(A @ np.linalg.solve(A, b) - b).max() / scale if len(b) else 0.0
    return rc, r_direct, r_numpy, A


def edge_terms(c, mu):
    """The library's own per-edge terms at the case's start: Haa, Hab, Hbb [E, 36], ga, gb [E, 6]."""
    E = len(c['edges'])
    out = np.zeros((E, 128))
    for e, (s, t) in enumerate(c['edges'].tolist()):
        Xs, Xt, T, L = (np.ascontiguousarray(a, dtype=np.float64) for a in (c['nodes'][s], c['nodes'][t], c['transforms'][e],
                                                                             c['informations'][e]))
        rc = lib().rdm_pose_graph_edge_terms_host(Xs.ctypes.data, Xt.ctypes.data, T.ctypes.data, L.ctypes.data,
                                                  ctypes.c_double(0.0 if mu is None else mu), int(c['uncertain'][e]), out[e].ctypes.data)
        assert rc == 0
    return out[:, 8:44], out[:, 44:80], out[:, 80:116], out[:, 116:122], out[:, 122:128]


_terms = {}


@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('name', list(GRAPHS))
def test_direct_host_solves_the_graph_s_system(name, lam):
    c, mu = graph(name), GRAPHS[name][1]
    n, edges = len(c['nodes']), c['edges']
    if name not in _terms:
        _terms[name] = edge_terms(c, mu)
    Haa, Hab, Hbb, ga, gb = _terms[name]
    D, b = np.zeros((n, 36)), np.zeros((n, 6))
    for e, (s, t) in enumerate(edges.tolist()):
        D[s] += Haa[e]
        D[t] += Hbb[e]
        b[s] += ga[e]
        b[t] += gb[e]
    diag, rhs = (1.0 + lam) * D, -b
    rc, r_direct, r_numpy, A = residuals(n, edges, diag, Hab, rhs)
    # the assembled matrix is the restatement's H + lam blockdiag(H)
    if (name, 'H') not in _terms:
        _terms[(name, 'H')] = R.normal_equations(c['nodes'], edges, c['transforms'], c['informations'], c['uncertain'], mu)[0][6:, 6:]
    H = _terms[(name, 'H')]
    want = H.copy()
    for i in range(n - 1):
        s = slice(6 * i, 6 * i + 6)
        want[s, s] += lam * H[s, s]
    assert np.abs(A - want).max() <= 1e-12 * np.abs(want).max()
    ev = np.linalg.eigvalsh(A) if len(A) <= 3000 else None  # (the 6 594 unknowns of `big` would take a minute)
    cond = ev[-1] / ev[0] if ev is not None else float('nan')
    print(f'{name:7s} lambda {lam:.0e} nodes {n} edges {len(edges)} direct {r_direct:.2e} numpy {r_numpy:.2e} condition {cond:.2e}')
    assert rc == 0
    assert r_direct <= max(10.0 * r_numpy, 1e-14)


# ---- 3. the smallest shapes at which the elimination can go wrong ---------------------------------------------------------------

def random_system(n, chords, seed):
    """A positive definite system on a chain of n nodes with chords: per node a positive definite 6 x 6 term, per edge a positive
    semi-definite 12 x 12 term J^T L J with J = [A | B] shaped like an edge's Jacobians on a 100 m scale (chain_system of
    tests/test_pose_graph_chain.py).  The chain edges alternate their direction and every second chord is stored target first, so
    both transposition conventions of `off` occur.  -> edges, diag, off, rhs."""
    rng = np.random.default_rng(seed)

    def jacobian():
        J = rng.normal(size=(6, 6))
        J[3:, :3] *= rng.uniform(1.0, cases.SCALE)
        return J

    edges = [((i, i + 1) if i % 2 else (i + 1, i)) for i in range(n - 1)] + [((s, t) if k % 2 else (t, s)) for k, (s, t) in enumerate(chords)]
    diag = np.zeros((n, 6, 6))
    off = np.zeros((len(edges), 6, 6))
    for i in range(n):
        J = jacobian()
        diag[i] = J.T @ cases.random_information(rng) @ J
    for e, (s, t) in enumerate(edges):
        A = jacobian()
        J = np.concatenate([A, -A + 0.1 * jacobian()], 1)
        M = J.T @ cases.random_information(rng) @ J
        M = 0.5 * (M + M.T)
        diag[s] += M[:6, :6]
        diag[t] += M[6:, 6:]
        off[e] = M[:6, 6:]
    diag = 0.5 * (diag + diag.transpose(0, 2, 1))
    rhs = rng.normal(size=(n, 6)) * 100.0
    return np.array(edges, np.int64), diag.reshape(n, 36), off.reshape(-1, 36), rhs


# name -> (nodes, chords, the separator the rule gives)
SHAPES = {
    'one free node': (2, [], []),
    'three nodes': (3, [], []),
    'separator at node 1': (5, [(1, 3)], [1]),
    'separator at the last node': (8, [(7, 2), (7, 4)], [7]),
    'adjacent separators': (14, [(3, 6), (3, 8), (4, 10), (4, 12)], [3, 4]),
    'chord between separators': (14, [(3, 6), (3, 8), (10, 5), (10, 12), (3, 10)], [3, 10]),
    # (random_system stores the two (3, 10) chords as (10, 3) and (3, 10): both transposition conventions in one Schur block)
    'double edge between separators': (14, [(3, 6), (3, 8), (10, 5), (10, 12), (3, 10), (3, 10)], [3, 10]),
    'three chords into three runs': (16, [(4, 1), (4, 7), (12, 9), (12, 15), (8, 2), (8, 6), (8, 10), (8, 14)], [4, 8, 12]),
    'two chords into one run': (12, [(2, 6), (2, 9)], [2]),
    'double edge on a chord': (10, [(2, 6), (2, 6)], [2]),
    'run of one node': (12, [(3, 7), (3, 9), (5, 1), (5, 11)], [3, 5]),
    'run longer than 256': (300, [(10, 290), (10, 150)], [10]),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_direct_host_on_the_small_shapes(name):
    n, chords, want = SHAPES[name]
    edges, diag, off, rhs = random_system(n, chords, seed=200 + n + len(chords))
    size, out = separator(n, edges)
    assert out[:size].tolist() == want
    rc, r_direct, r_numpy, A = residuals(n, edges, diag, off, rhs)
    print(f'{name}: direct {r_direct:.2e} numpy {r_numpy:.2e} condition {np.linalg.cond(A):.2e}')
    assert rc == 0
    assert r_direct <= max(10.0 * r_numpy, 1e-14)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------

def test_direct_host_refuses_pivots_that_are_not_positive():
    n, chords, _ = SHAPES['chord between separators']
    edges, diag, off, rhs = random_system(n, chords, seed=77)
    assert direct_host(n, edges, diag, off, rhs)[0] == 0
    bad = diag.copy()
    bad[6] = -bad[6]  # inside a run
    rc, _ = direct_host(n, edges, bad, off, rhs)
    assert rc == -1 and 'not positive' in lib().rdm_last_error().decode()
    weak = diag.copy()
    weak[10] = 1e-6 * np.eye(6).reshape(36)  # a separator node: positive by itself, indefinite once Y^T Y is taken away
    rc, _ = direct_host(n, edges, weak, off, rhs)
    assert rc == -1 and 'not positive' in lib().rdm_last_error().decode() and 'Schur' in lib().rdm_last_error().decode()


def over_the_cap():
    """A chain with max_separator + 1 disjoint chords (3 k + 1, 3 k + 3): every chord needs a node of its own."""
    k = lib().rdm_pose_graph_direct_max_separator() + 1
    n = 3 * k + 4
    edges = [(i + 1, i) for i in range(n - 1)] + [(3 * j + 1, 3 * j + 3) for j in range(k)]
    return n, np.array(edges, np.int64), k


def test_workspace_bytes_refuses_a_graph_over_the_cap():
    L = lib()
    cap = L.rdm_pose_graph_direct_max_separator()
    assert cap >= 256
    n, edges, k = over_the_cap()
    assert separator(n, edges)[0] == k
    noff, eoff = np.array([0, n], np.int64), np.array([0, len(edges)], np.int64)
    assert L.rdm_pose_graph_workspace_bytes_ls(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data, 0, 1) == 0
    msg = L.rdm_last_error().decode()
    print(msg)
    assert str(k) in msg and str(cap) in msg and 'graph 0' in msg
    for pre in (0, 1):
        assert L.rdm_pose_graph_workspace_bytes_ls(1, noff.ctypes.data, eoff.ctypes.data, edges.ctypes.data, pre, 0) == \
            L.rdm_pose_graph_workspace_bytes_pc(1, n, len(edges), pre) > 0
    # one chord fewer fits, and the direct solve's workspace holds more than the conjugate gradients'
    fits = edges[:-1]
    eoff[1] = len(fits)
    size = L.rdm_pose_graph_workspace_bytes_ls(1, noff.ctypes.data, eoff.ctypes.data, fits.ctypes.data, 0, 1)
    assert size > L.rdm_pose_graph_workspace_bytes_pc(1, n, len(fits), 1) + 36 * 8 * cap * cap
    assert L.rdm_pose_graph_workspace_bytes_ls(1, noff.ctypes.data, eoff.ctypes.data, fits.ctypes.data, 0, 2) == 0


# ---- 5. arguments -------------------------------------------------------------------------------------------------------------

def test_unknown_linear_solver_is_a_value_error_before_any_gpu_work():
    from rdmnet_amd import ops
    c = cases.consistent('ring3')
    with pytest.raises(ValueError, match='nonsense'):
        ops.pose_graph_optimize(c['nodes'], c['edges'], c['transforms'], c['informations'], linear_solver='nonsense')
    assert ops.POSE_GRAPH_LINEAR_SOLVERS == {'pcg': 0, 'direct': 1}


def test_command_line_offers_the_linear_solver():
    from rdmnet_amd import trajectory
    ap = trajectory.make_parser()
    assert ap.parse_args(['--features-root', 'x']).linear_solver == 'pcg'
    assert ap.parse_args(['--features-root', 'x', '--optimize', '--linear-solver', 'direct']).linear_solver == 'direct'
    with pytest.raises(SystemExit):
        ap.parse_args(['--features-root', 'x', '--linear-solver', 'nonsense'])
