"""Cross covariances and loop-edge consistency of a pose graph, restated densely ("cross covariances").  What
rdm_pose_graph_consistency / ops.pose_graph_consistency and the host twins are held against; it shares no code with them.  From the
long-double inverse of pose_graph_marginals_restatement (node 0's rows and columns zero) it takes the off-diagonal blocks Sigma_st,
and with pose_graph_restatement's exact Jacobians A, B of a pair's residual r
    M  = A Sigma_ss A^T + A Sigma_st B^T + B Sigma_ts A^T + B Sigma_tt B^T
    d2 = r^T (M + L^-1)^-1 r          (without L: r^T M^-1 r)
in long double.  The same quantities from np.linalg.inv's blocks in float64 are the yardstick, as for the marginals:
    Sigma_st   max|got - R| / sqrt(max|R_ss| max|R_tt|) <= max(10 x numpy's, 1e-14)   (the geometric mean bounds |Sigma_st| by
               Cauchy-Schwarz, so a small cross block does not inflate the error)
    M          max|got - R| / max|R|                    <= max(10 x numpy's, 1e-14)
    d2         |got - R| / R                            <= max(10 x numpy's, 1e-12)
each the largest over the pairs of a call."""
import numpy as np

import pose_graph_marginals_restatement as M
import pose_graph_restatement as R


def longdouble_inverse(A):
    """The inverse of a symmetric positive definite matrix in np.longdouble by a Gauss-Jordan elimination in place, without pivoting
    (the same elimination as pose_graph_marginals_restatement's on [A | I], at half its work)."""
    W = np.array(A, dtype=np.longdouble)
    for k in range(len(W)):
        row = W[k] / W[k, k]
        row[k] = 1 / W[k, k]
        col = W[:, k].copy()
        col[k] = 0
        W[:, k] = 0
        W -= col[:, None] * row[None, :]
        W[k] = row
    return W


def current_transform(Xs, Xt):
    """X_t^-1 X_s with the closed-form inverse."""
    T = np.eye(4)
    T[:3, :3] = Xt[:3, :3].T @ Xs[:3, :3]
    T[:3, 3] = Xt[:3, :3].T @ (Xs[:3, 3] - Xt[:3, 3])
    return T


class Reference:
    """Of the dense free-node matrix A [6 (n - 1), 6 (n - 1)] of a graph of n nodes: the long-double inverse and np.linalg.inv's,
    both [6 n, 6 n] with node 0's rows and columns zero."""

    def __init__(self, A):
        m = len(A)
        self.exact = np.zeros((m + 6, m + 6), np.longdouble)
        self.numpy = np.zeros((m + 6, m + 6))
        if m:
            self.exact[6:, 6:] = longdouble_inverse(A)
            self.numpy[6:, 6:] = np.linalg.inv(A)

    @staticmethod
    def block(inv, s, t):
        return inv[6 * s:6 * s + 6, 6 * t:6 * t + 6]

    def cross(self, pairs):
        """-> the long-double Sigma_st [P, 6, 6] rounded to float64."""
        return np.stack([np.asarray(self.block(self.exact, s, t), dtype=np.float64) for s, t in pairs]) if len(pairs) else np.zeros((0, 6, 6))

    def cross_error(self, pairs, got):
        worst = 0.0
        for k, (s, t) in enumerate(pairs):
            if s == 0 or t == 0:
                assert np.all(got[k] == 0.0), f'pair {k} ({s}, {t}) holds node 0: its block is zero'
                continue
            ref = np.asarray(self.block(self.exact, s, t), dtype=np.float64)
            scale = np.sqrt(float(np.abs(self.block(self.exact, s, s)).max()) * float(np.abs(self.block(self.exact, t, t)).max()))
            worst = max(worst, float(np.abs(got[k] - ref).max()) / scale)
        return worst

    def check_cross(self, name, pairs, got):
        """got [P, 6, 6] against the criterion.  -> (error, numpy's)."""
        pairs = np.asarray(pairs).reshape(-1, 2).tolist()
        got = np.asarray(got, dtype=np.float64).reshape(-1, 6, 6)
        assert len(got) == len(pairs) and np.all(np.isfinite(got))
        err = self.cross_error(pairs, got)
        ynp = self.cross_error(pairs, np.stack([self.block(self.numpy, s, t) for s, t in pairs])) if pairs else 0.0
        bound = max(10.0 * ynp, 1e-14)
        print(f'{name}: pairs {len(pairs)} cross {err:.2e} numpy {ynp:.2e} ratio {err / ynp if ynp > 0 else float("nan"):.2f} bound {bound:.2e}')
        assert err <= bound, f'{name}: cross {err:.3e} > {bound:.3e}'
        return err, ynp

    def terms(self, inv, nodes, pairs, transforms, informations):
        """-> (r [P, 6], M [P, 6, 6], d2 [P]) from the blocks of `inv`, in its precision."""
        kind = inv.dtype
        rs, Ms, ds = [], [], []
        for k, (s, t) in enumerate(pairs):
            r, A, B = R.jacobians(nodes[s], nodes[t], transforms[k])
            A, B, r = A.astype(kind), B.astype(kind), r.astype(kind)
            Sst = self.block(inv, s, t)
            Mk = A @ self.block(inv, s, s) @ A.T + A @ Sst @ B.T + B @ Sst.T @ A.T + B @ self.block(inv, t, t) @ B.T
            K = Mk.copy()
            if informations is not None:
                L = R.sym(informations[k]).astype(kind)
                K = K + (longdouble_inverse(L) if kind == np.longdouble else np.linalg.inv(L))
            z = longdouble_inverse(K) @ r if kind == np.longdouble else np.linalg.solve(K, r)
            rs.append(r)
            Ms.append(Mk)
            ds.append(r @ z)
        return np.array(rs), np.array(Ms), np.array(ds)

    def check_terms(self, name, nodes, pairs, transforms, informations, got_m, got_d2=None):
        """The pairs' M [P, 6, 6] and d2 [P] (None: M alone, for residuals that are zero up to rounding) against the criteria.
        -> (M's error, numpy's, d2's error, numpy's)."""
        pairs = np.asarray(pairs).reshape(-1, 2).tolist()
        got_m = np.asarray(got_m, dtype=np.float64).reshape(-1, 6, 6)
        with_d2, got_d2 = got_d2 is not None, np.asarray(np.ones(len(pairs)) if got_d2 is None else got_d2, dtype=np.float64).reshape(-1)
        assert len(got_m) == len(pairs) == len(got_d2) and np.all(np.isfinite(got_m)) and np.all(np.isfinite(got_d2))
        _, Me, de = self.terms(self.exact, nodes, pairs, transforms, informations)
        _, Mn, dn = self.terms(self.numpy, nodes, pairs, transforms, informations)
        Me, de = Me.astype(np.float64), de.astype(np.float64)
        for k in range(len(pairs)):
            assert np.array_equal(got_m[k], got_m[k].T), f'M of pair {k} is not exactly symmetric'
        scale = np.abs(Me).reshape(len(pairs), -1).max(1)
        err_m = float((np.abs(got_m - Me).reshape(len(pairs), -1).max(1) / scale).max())
        np_m = float((np.abs(Mn - Me).reshape(len(pairs), -1).max(1) / scale).max())
        err_d = float((np.abs(got_d2 - de) / de).max()) if with_d2 else 0.0
        np_d = float((np.abs(dn - de) / de).max()) if with_d2 else 0.0
        bound_m, bound_d = max(10.0 * np_m, 1e-14), max(10.0 * np_d, 1e-12)
        print(f'{name}: pairs {len(pairs)} M {err_m:.2e} numpy {np_m:.2e} ratio {err_m / np_m if np_m > 0 else float("nan"):.2f} bound '
              f'{bound_m:.2e}; d2 {err_d:.2e} numpy {np_d:.2e} ratio {err_d / np_d if np_d > 0 else float("nan"):.2f} bound {bound_d:.2e} '
              f'(d2 from {de.min():.3g} to {de.max():.3g})')
        assert err_m <= bound_m, f'{name}: M {err_m:.3e} > {bound_m:.3e}'
        assert err_d <= bound_d, f'{name}: d2 {err_d:.3e} > {bound_d:.3e}'
        return err_m, np_m, err_d, np_d


_cache = {}


def graph(name):
    """One of pose_graph_marginals_restatement's GRAPHS with its pairs: all ordered pairs for the five graphs up to ring40 (at most
    50 nodes); for noisy, gross and noisy100 their loop edges (with their own transforms and informations) plus 200 seeded pairs.  A
    pair that is not an edge carries X_t^-1 X_s of the case's poses moved by up to 0.02 rad and 0.1 m, and a random information matrix.
    -> (case, weights, Reference, pairs [P, 2], transforms [P, 4, 4], informations [P, 6, 6]), computed once and left unchanged."""
    if name not in _cache:
        import pose_graph_cases as cases
        c, w, ref = M.graph(name)
        n = len(c['nodes'])
        rng = np.random.default_rng(900 + n)
        loops = []
        if n <= 50:
            pairs = [(s, t) for s in range(n) for t in range(n) if s != t]
        else:
            loops = [e for e in range(len(c['edges'])) if c['uncertain'][e]]
            pairs = [tuple(c['edges'][e]) for e in loops]
            while len(pairs) < len(loops) + 200:
                s, t = (int(v) for v in rng.integers(0, n, size=2))
                if s != t:
                    pairs.append((s, t))
        T = np.stack([R.retract(current_transform(c['nodes'][s], c['nodes'][t]), cases.perturbation(rng, 0.02, 0.1)) for s, t in pairs])
        L = np.stack([cases.random_information(rng) for _ in pairs])
        for k, e in enumerate(loops):
            T[k], L[k] = c['transforms'][e], c['informations'][e]
        _cache[name] = (c, w, Reference(ref.A), np.array(pairs, np.int64), T, L)
    return _cache[name]
