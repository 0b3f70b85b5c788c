"""Marginal covariances of a pose graph, restated densely ("marginal covariances").  The definition that
rdm_pose_graph_marginals / ops.pose_graph_marginals are held against; it shares no code with them: H = sum_e w_e J_e^T L_e J_e is
assembled densely from pose_graph_restatement's exact Jacobians with explicit weights, and inverted in np.longdouble by a
Gauss-Jordan elimination written here.  Sigma_i is the 6 x 6 diagonal block of H^-1 over the free nodes 1 .. n - 1 (node 0 fixed).

The accuracy criterion (the same for the host twin and the GPU): the largest per-block relative error
max_i max|S_i - R_i| / max|R_i| against the long-double blocks R is at most max(10 x the same error of np.linalg.inv on the same
matrix, 1e-14).  numpy is the yardstick -- these graphs have condition numbers up to 1e12 and no float64 method gives their
covariances to a fixed tolerance --, the factor 10 is the margin of a hand-written block elimination against LAPACK
(tests/test_pose_graph_direct.py), the floor covers the well-conditioned tiny cases."""
import numpy as np

import pose_graph_cases as cases
import pose_graph_restatement as R


def information(nodes, edges, transforms, informations, weights=None):
    """H [6 n, 6 n] (rows of node 0 included) with explicit per-edge weights (None: ones)."""
    n = len(nodes)
    H = np.zeros((6 * n, 6 * n))
    for e, (s, t) in enumerate(np.asarray(edges).reshape(-1, 2).tolist()):
        _, A, B = R.jacobians(nodes[s], nodes[t], transforms[e])
        L = R.sym(informations[e])
        w = 1.0 if weights is None else float(weights[e])
        ss, tt = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[ss, ss] += w * (A.T @ L @ A)
        H[ss, tt] += w * (A.T @ L @ B)
        H[tt, ss] += w * (B.T @ L @ A)
        H[tt, tt] += w * (B.T @ L @ B)
    return H


def longdouble_inverse(A):
    """Gauss-Jordan without pivoting (A is symmetric positive definite) in np.longdouble."""
    n = len(A)
    M = np.concatenate([np.asarray(A, dtype=np.longdouble), np.eye(n, dtype=np.longdouble)], axis=1)
    for k in range(n):
        M[k] /= M[k, k]
        col = M[:, k].copy()
        col[k] = 0
        M -= col[:, None] * M[k][None, :]
    return M[:, n:]


def diagonal_blocks(M):
    m = len(M) // 6
    return np.stack([np.asarray(M[6 * i:6 * i + 6, 6 * i:6 * i + 6], dtype=np.float64) for i in range(m)]) if m else np.zeros((0, 6, 6))


def block_error(got, ref):
    """The largest per-block relative error of got [m, 6, 6] against ref."""
    if len(ref) == 0:
        return 0.0
    return float((np.abs(got - ref).reshape(len(ref), -1).max(1) / np.abs(ref).reshape(len(ref), -1).max(1)).max())


class Reference:
    """Of a dense free-node matrix A [6 m, 6 m]: blocks (the long-double marginals, rounded to float64), numpy_error (np.linalg.inv's
    block error against them) and bound, the criterion's right-hand side."""

    def __init__(self, A):
        self.A = A
        self.blocks = diagonal_blocks(longdouble_inverse(A))
        self.numpy_error = block_error(diagonal_blocks(np.linalg.inv(A)), self.blocks) if len(A) else 0.0
        self.bound = max(10.0 * self.numpy_error, 1e-14)

    def check(self, name, covariances):
        """covariances [m + 1, 6, 6] with row 0 the fixed node's: structure and the accuracy criterion.  -> the error."""
        cov = np.asarray(covariances, dtype=np.float64).reshape(-1, 6, 6)
        assert len(cov) == len(self.blocks) + 1
        assert np.all(cov[0] == 0.0), 'row 0 is the fixed node'
        assert np.all(np.isfinite(cov))
        for i in range(1, len(cov)):
            assert np.array_equal(cov[i], cov[i].T), f'block {i} is not exactly symmetric'
            assert np.all(np.diag(cov[i]) > 0.0), f'block {i} has a diagonal entry that is not positive'
        err = block_error(cov[1:], self.blocks)
        ratio = err / self.numpy_error if self.numpy_error > 0 else float('nan')
        print(f'{name}: nodes {len(cov)} marginals {err:.2e} numpy {self.numpy_error:.2e} ratio {ratio:.2f} bound {self.bound:.2e}')
        assert err <= self.bound, f'{name}: {err:.3e} > {self.bound:.3e}'
        return err


# name -> (case, mu of the line process whose weights at the case's start poses are the edge weights; None: ones)
GRAPHS = {
    'pair': (lambda: cases.consistent('pair'), None),
    'ring3': (lambda: cases.consistent('ring3'), None),
    'double': (lambda: cases.consistent('double'), None),
    'tree': (lambda: cases.tree(), None),
    'ring40': (lambda: cases.consistent('ring40'), None),
    'noisy': (lambda: cases.noisy(), 1.0),
    'gross': (lambda: cases.noisy(gross=3), 1.0),
    'noisy100': (lambda: cases.noisy(n=100, loops=16), 1.0),
}
_cache = {}


def graph(name):
    """-> (case, weights [E], Reference of its H over the free nodes), computed once and left unchanged."""
    if name not in _cache:
        c, mu = GRAPHS[name][0](), GRAPHS[name][1]
        w = R.weights(c['nodes'], c['edges'], c['transforms'], c['informations'], c['uncertain'], mu)
        H = information(c['nodes'], c['edges'], c['transforms'], c['informations'], w)
        _cache[name] = (c, w, Reference(H[6:, 6:]))
    return _cache[name]


def closed_form():
    """One edge (1 -> 0) at zero residual: A = I, so H = L and Sigma_1 = L^-1.  -> (case, the information matrix)."""
    rng = np.random.default_rng(41)
    X0, T = np.eye(4), cases.random_pose(rng, scale=5.0)
    L = cases.random_information(rng)
    c = dict(nodes=np.stack([X0, X0 @ T]), edges=np.array([[1, 0]], np.int64), transforms=T[None], informations=L[None],
             uncertain=np.zeros(1, np.uint8))
    return c, L
