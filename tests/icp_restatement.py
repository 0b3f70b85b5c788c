"""Float64 numpy restatement of point-to-point ICP as rdm_icp_point_to_point defines it (Open3D's RegistrationICP with
TransformationEstimationPointToPoint and ICPConvergenceCriteria; parity with Open3D itself is unpinned).

Neighbour step, to the bit: targets are float32 read as double, d = q - t per axis, d2 = ((dx*dx) + (dy*dy)) + (dz*dz),
accept iff d2 < r2 with r2 = (double)(float)(r*r), ties in d2 to the lowest target index.  Candidates come from a
cKDTree; every candidate in the ball is looked at whenever the k nearest could hide a tie.  Transforms are applied
row by row as ((R0*x + R1*y) + R2*z) + t, as the kernel does (numpy's elementwise arithmetic is never contracted).
The Kabsch step is numpy's SVD with the reflection fix."""
import numpy as np
from scipy.spatial import cKDTree

IDENTITY12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float64)


def search_r2(r):
    return float(np.float32(r * r))


class Target:
    def __init__(self, target, r, workers=16):
        self.t = np.asarray(target, dtype=np.float32)[:, :3].astype(np.float64)
        self.r2 = search_r2(r)
        self.R = np.sqrt(self.r2) * (1 + 1e-7)
        self.tree = cKDTree(self.t) if len(self.t) else None
        self.workers = workers

    def _exact(self, q, cand):
        d = q[:, None, :] - self.t[cand]
        return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])

    def correspondences(self, pcd, k=8):
        """-> idx int32 [n] (-1 = none), d2 float64 [n] (-1 where idx is -1), and the near-miss flags
        (restated d2 within 1e-9 of r2, or the two nearest targets within 1e-9 of each other)."""
        pcd = np.asarray(pcd, dtype=np.float64)
        n, m = len(pcd), len(self.t)
        idx = np.full(n, -1, np.int32)
        d2 = np.full(n, -1.0)
        near = np.zeros(n, bool)
        if n == 0 or m == 0:
            return idx, d2, near
        k = min(k, m)
        fin = np.isfinite(pcd).all(1)
        q = np.where(fin[:, None], pcd, 0.0)
        dist, ii = self.tree.query(q, k=k, distance_upper_bound=self.R, workers=self.workers)
        dist, ii = dist.reshape(n, k), ii.reshape(n, k)
        valid = (ii < m) & fin[:, None]
        safe = np.where(valid, ii, 0)
        e = self._exact(q, safe)
        e = np.where(valid, e, np.inf)
        acc = np.where(e < self.r2, e, np.inf)
        best = acc.min(1)
        bj = np.where(acc == best[:, None], safe, np.iinfo(np.int64).max).min(1)
        got = np.isfinite(best)
        idx[got] = bj[got]
        d2[got] = best[got]
        srt = np.sort(e, 1)
        with np.errstate(invalid='ignore'):  # (inf - inf where there are no candidates)
            near = (np.abs(srt[:, 0] - self.r2) <= 1e-9) | (
                (k > 1) & (np.abs(srt[:, min(1, k - 1)] - srt[:, 0]) <= 1e-9))
        # the k nearest may hide further candidates tied with the best: look at the whole ball there
        full = valid[:, -1] & (dist[:, -1] ** 2 <= np.where(got, best, self.r2) * (1 + 1e-9) + 1e-12)
        for i in np.nonzero(full)[0]:
            cand = np.asarray(self.tree.query_ball_point(q[i], self.R), dtype=np.int64)
            ee = self._exact(q[i:i + 1], cand)[0]
            ok = ee < self.r2
            if ok.any():
                b = ee[ok].min()
                idx[i] = cand[ok][ee[ok] == b].min()
                d2[i] = b
        return idx, d2, near


def apply(M, p):
    """M: 12 (R|t rows) or 4x4; p [n, 3] float64 -> M . p with the kernel's expression order."""
    M = np.asarray(M, dtype=np.float64).reshape(-1)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((M[4 * a] * x + M[4 * a + 1] * y) + M[4 * a + 2] * z) + M[4 * a + 3] for a in range(3)], 1)


def compose(U, T):
    """update (12) . transformation (4x4) -> 4x4, the kernel's order."""
    U = np.asarray(U, dtype=np.float64).reshape(-1)
    out = T.copy()
    for a in range(3):
        for b in range(4):
            out[a, b] = ((U[4 * a] * T[0, b] + U[4 * a + 1] * T[1, b]) + U[4 * a + 2] * T[2, b]) + U[4 * a + 3] * T[3, b]
    return out


def kabsch(p, t):
    """Rigid R|t (12 values) that maps p onto t in the least-squares sense; the identity without points."""
    if len(p) == 0:
        return IDENTITY12.copy()
    ms, mt = p.mean(0), t.mean(0)
    H = (p - ms).T @ (t - mt)
    U, _, Vt = np.linalg.svd(H)
    s = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, s]) @ U.T
    tt = mt - R @ ms
    return np.concatenate([R, tt[:, None]], 1).reshape(-1)


def evaluate(tgt, pcd, n_source):
    idx, d2, near = tgt.correspondences(pcd)
    ok = idx >= 0
    n = int(ok.sum())
    fitness = n / n_source if n else 0.0
    rmse = float(np.sqrt(d2[ok].sum() / n)) if n else 0.0
    return idx, d2, near, n, fitness, rmse


def icp(source, target, r, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> (transformation 4x4, fitness, rmse, n_corr, iterations)."""
    src = np.asarray(source, dtype=np.float32)[:, :3].astype(np.float64)
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    pcd = src if np.array_equal(T, np.eye(4)) else apply(T, src)
    tgt = Target(target, r)
    if len(src) == 0:
        return T, 0.0, 0.0, 0, 0
    idx, _, _, n, fit, rmse = evaluate(tgt, pcd, len(src))
    it = 0
    for it in range(1, max_iteration + 1):
        ok = idx >= 0
        U = kabsch(pcd[ok], tgt.t[idx[ok]])
        T = compose(U, T)
        pcd = apply(U, pcd)
        idx, _, _, n2, fit2, rmse2 = evaluate(tgt, pcd, len(src))
        conv = abs(fit - fit2) < relative_fitness and abs(rmse - rmse2) < relative_rmse
        n, fit, rmse = n2, fit2, rmse2
        if conv:
            break
    return T, fit, rmse, n, it
