"""The odometry-chain preconditioner of the pose-graph solve, on the host: the kernels' factor and apply
functions compiled for the host (rdm_pose_graph_chain_host) against np.linalg.solve; a numpy restatement of the preconditioner M,
written here from the restatement's normal equations, is symmetric positive definite on the test graphs; the option's argument
check.  No GPU."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_restatement as R

LAMBDA = 1e-6  # the solve's first damping


# ---- rdm_pose_graph_chain_host ------------------------------------------------------------------------------------------------

def chain_system(n, seed):
    """A block tridiagonal M that is positive definite by construction: per pair (i, i + 1) a positive semi-definite 12 x 12 term
    J^T L J with J = [A | B] shaped like an edge's Jacobians on a 100 m scale (the translation rows see the rotation columns
    through a lever arm of up to 100 m), plus per node a positive definite 6 x 6 term (what edges to node 0 or to far nodes leave
    on the diagonal).  -> diag [n, 36], off [n - 1, 36] (blocks (i, i + 1)), M dense."""
    rng = np.random.default_rng(seed)

    def jacobian():
        J = rng.normal(size=(6, 6))
        J[3:, :3] *= rng.uniform(1.0, cases.SCALE)
        return J

    M = np.zeros((6 * n, 6 * n))
    for i in range(n):
        J = jacobian()
        M[6 * i:6 * i + 6, 6 * i:6 * i + 6] += J.T @ cases.random_information(rng) @ J
    for i in range(n - 1):
        A = jacobian()
        J = np.concatenate([A, -A + 0.1 * jacobian()], 1)
        M[6 * i:6 * i + 12, 6 * i:6 * i + 12] += J.T @ cases.random_information(rng) @ J
    M = 0.5 * (M + M.T)
    diag = np.stack([M[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n)]).reshape(n, 36)
    off = np.stack([M[6 * i:6 * i + 6, 6 * i + 6:6 * i + 12] for i in range(n - 1)]).reshape(n - 1, 36) if n > 1 else np.zeros((0, 36))
    return np.ascontiguousarray(diag), np.ascontiguousarray(off), M


def chain_host(diag, off, rhs):
    from rdmnet_amd import _lib
    L = _lib.lib()
    out = np.full_like(rhs, np.nan)
    rc = L.rdm_pose_graph_chain_host(len(diag), diag.ctypes.data, off.ctypes.data if len(off) else 0, rhs.ctypes.data, out.ctypes.data)
    return rc, out


@pytest.mark.parametrize('n', [1, 2, 3, 50, 300])
def test_chain_host_equals_numpy_solve(n):
    """1e-9 of the solution's largest entry.  Both solvers are backward stable, so each is off the exact solution by about
    cond(M) 2^-53 relative; the condition number is computed and printed, and the bound must hold with it."""
    diag, off, M = chain_system(n, seed=100 + n)
    rng = np.random.default_rng(n)
    rhs = np.ascontiguousarray(rng.normal(size=(n, 6)) * 100.0)
    rc, got = chain_host(diag, off, rhs)
    assert rc == 0
    want = np.linalg.solve(M, rhs.reshape(-1)).reshape(n, 6)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('n', n, 'relative error', err, 'condition number', np.linalg.cond(M), 'smallest eigenvalue', np.linalg.eigvalsh(M)[0])
    assert err <= 1e-9


def test_chain_host_refuses_an_indefinite_block():
    diag, off, _ = chain_system(5, seed=9)
    rhs = np.ones((5, 6))
    assert chain_host(diag, off, rhs)[0] == 0
    bad = diag.copy()
    bad[3] = -bad[3]
    from rdmnet_amd import _lib
    rc, _ = chain_host(bad, off, rhs)
    assert rc == -1 and 'not positive' in _lib.lib().rdm_last_error().decode()
    # indefinite only after the chain's update: a diagonal block smaller than what the block before it takes away
    weak = diag.copy()
    weak[4] = 1e-6 * np.eye(6).reshape(36)
    assert chain_host(weak, off, rhs)[0] == -1


# ---- the preconditioner, restated ---------------------------------------------------------------------------------------------

def chain_preconditioner(c, mu=None, lam=LAMBDA):
    """-> (A, M) over the free nodes 1 .. n - 1 at the case's start: A = H + lam blockdiag(H), and M: A's diagonal blocks and its
    blocks between nodes i and i + 1 (H's block there IS the sum of l A^T L B, or its transpose, over the edges that join the two)."""
    H, _ = R.normal_equations(c['nodes'], c['edges'], c['transforms'], c['informations'], c['uncertain'], mu)
    H = H[6:, 6:]
    m = len(c['nodes']) - 1
    M = np.zeros_like(H)
    D = np.zeros_like(H)
    for i in range(m):
        s = slice(6 * i, 6 * i + 6)
        D[s, s] = H[s, s]
        M[s, s] = (1.0 + lam) * H[s, s]
        if i + 1 < m:
            t = slice(6 * i + 6, 6 * i + 12)
            M[s, t] = H[s, t]
            M[t, s] = H[s, t].T
    return H + lam * D, M


GRAPHS = [('tree', lambda: cases.tree(), None), ('noisy', lambda: cases.noisy(), 1.0), ('gross', lambda: cases.noisy(gross=3), 1.0),
          ('double', lambda: cases.consistent('double'), None), ('hub', lambda: cases.consistent('hub'), None),
          ('ring40', lambda: cases.consistent('ring40'), None)]


@pytest.mark.parametrize('name,make,mu', GRAPHS, ids=[g[0] for g in GRAPHS])
def test_restated_preconditioner_is_symmetric_positive_definite(name, make, mu):
    c = make()
    A, M = chain_preconditioner(c, mu)
    assert np.array_equal(M, M.T) or np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    low = np.linalg.eigvalsh(0.5 * (M + M.T))[0]
    print(name, 'smallest eigenvalue of M', low, 'of A', np.linalg.eigvalsh(A)[0])
    assert low > 0.0
    if name == 'tree':  # a chain and nothing else: the preconditioner is the system
        assert np.array_equal(M, A) or np.abs(M - A).max() <= 1e-15 * np.abs(A).max()


def test_chain_host_solves_a_graph_s_preconditioner():
    """The host functions on the M of a real graph (the 40-ring with chords, whose chain edges are (i + 1, i)): the blocks are cut
    out of the restated M, so the block order and the transposition convention of `off` are held too."""
    c = cases.consistent('ring40')
    _, M = chain_preconditioner(c)
    m = len(c['nodes']) - 1
    diag = np.ascontiguousarray(np.stack([M[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(m)]).reshape(m, 36))
    off = np.ascontiguousarray(np.stack([M[6 * i:6 * i + 6, 6 * i + 6:6 * i + 12] for i in range(m - 1)]).reshape(m - 1, 36))
    rhs = np.ascontiguousarray(np.random.default_rng(5).normal(size=(m, 6)))
    rc, got = chain_host(diag, off, rhs)
    want = np.linalg.solve(M, rhs.reshape(-1)).reshape(m, 6)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('relative error', err, 'condition number', np.linalg.cond(M))
    assert rc == 0 and err <= 1e-9


# ---- arguments ----------------------------------------------------------------------------------------------------------------

def test_unknown_preconditioner_is_a_value_error_before_any_gpu_work():
    from rdmnet_amd import ops
    c = cases.consistent('ring3')
    with pytest.raises(ValueError, match='nonsense'):
        ops.pose_graph_optimize(c['nodes'], c['edges'], c['transforms'], c['informations'], preconditioner='nonsense')
    assert ops.POSE_GRAPH_PRECONDITIONERS == {'block_jacobi': 0, 'chain': 1}


def test_command_line_offers_the_preconditioner():
    from rdmnet_amd import trajectory
    ap = trajectory.make_parser()
    assert ap.parse_args(['--features-root', 'x']).preconditioner == 'block_jacobi'
    assert ap.parse_args(['--features-root', 'x', '--optimize', '--preconditioner', 'chain']).preconditioner == 'chain'
    with pytest.raises(SystemExit):
        ap.parse_args(['--features-root', 'x', '--preconditioner', 'nonsense'])
