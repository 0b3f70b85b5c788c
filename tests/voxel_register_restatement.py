"""NumPy restatement (float64) of the scan-to-map registration on the per-voxel Gaussians (include/rdmnet_hip.h, "voxel map
registration"), written from the definition and sharing no code with the library.  The map is a
voxel_moments_restatement.Moments: sorted keys, counts, the C sums and the nine moment sums.

One evaluation of a scan at the pose X = (R, t):
  gate      each row as the map's integrate does (non-finite among its C values, then range), w = X p with its association,
            Q_d = floor(w_d / voxel 2^20), cell_d = Q_d >> 20; a point the map would count in out_of_extent is dropped;
  visit     cell + o for o = (0,0,0), (-1,0,0), (+1,0,0), (0,-1,0), (0,+1,0), (0,0,-1), (0,0,+1) (neighbors = 1: the first only),
            passing over a cell outside [-2^20, 2^20); a voxel takes part if it is in the map with n >= min_points points;
  per pair  mu_d = (sum_d / n) / 2^20 voxel, Sigma = the moments' covariance + sigma^2 I, M = Sigma^-1 (numpy.linalg.inv),
            r = w - mu, q = w - t, J = [-[q]x | I3];
  totals    H = sum J^T M J, g = sum J^T M r, cost = sum r^T M r, n_corr = the number of pairs.
Iteration: evaluate; stop with status 0 once max_iteration updates are applied; solve H delta = -g by a Cholesky factorisation
without pivoting, status 2 if n_corr = 0 or a pivot is <= 0 or not finite; else R <- Exp(omega) R, t <- t + v with delta =
(omega, v); if |omega| < rot_eps and |v| < trans_eps evaluate once more and stop with status 1."""
import numpy as np

import voxel_moments_restatement as MR

SCALE = 1048576.0
HALF = 1 << 20
OFFSETS = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)


def skew(v):
    """[K, 3] -> [v]x as [K, 3, 3]."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def exp_so3(omega):
    """Rodrigues: I + sin(th) / th [w]x + (1 - cos(th)) / th^2 [w]x^2 (the series of the two factors below 1e-4)."""
    omega = np.asarray(omega, np.float64)
    th2 = float(omega @ omega)
    th = np.sqrt(th2)
    a, b = (1.0 - th2 / 6.0, 0.5 - th2 / 24.0) if th < 1e-4 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    K = skew(omega)[0]
    return np.eye(3) + a * K + b * (K @ K)


def world_points(table, cloud, X, min_range=0.0, max_range=np.inf):
    """The gates, the transform and the cells of the points that pass -> (w float64 [K, 3], cells int64 [K, 3])."""
    C = table.map.channels
    p = np.asarray(cloud, np.float32)[:, :C].astype(np.float64)
    X = np.asarray(X, np.float64)
    voxel = np.float64(table.voxel)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        keep = np.isfinite(p).all(1)
        r2 = (x * x + y * y) + z * z
        keep &= (np.float64(min_range) * np.float64(min_range) <= r2) & (r2 <= np.float64(max_range) * np.float64(max_range))
        w = np.stack([((X[d, 0] * x + X[d, 1] * y) + X[d, 2] * z) + X[d, 3] for d in range(3)], 1)
        f = np.floor(w / voxel * SCALE)
        keep &= ((f >= -2.0 ** 40) & (f < 2.0 ** 40)).all(1)
        keep &= (np.abs(p[:, 3:]) < SCALE).all(1)
    w, f = w[keep], f[keep]
    return w, f.astype(np.int64) >> 20


def pairs(table, cells, min_points, neighbors):
    """-> (point index [P], map row [P]) of the point-voxel pairs, ordered by point and then by offset."""
    assert neighbors in (1, 7)
    c = cells[:, None, :] + OFFSETS[None, :neighbors, :]
    inside = ((c >= -HALF) & (c < HALF)).all(2)
    cc = np.where(inside[:, :, None], c, 0) + HALF
    key = (cc[:, :, 0].astype(np.uint64) << np.uint64(42)) | (cc[:, :, 1].astype(np.uint64) << np.uint64(21)) | cc[:, :, 2].astype(np.uint64)
    keys = table.keys
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    hit = inside & (keys[pos] == key) & (table.map.counts[pos] >= int(min_points))
    i, o = np.nonzero(hit)
    return i, pos[i, o]


def evaluate(table, cloud, X, sigma=0.02, min_points=4, neighbors=1, min_range=0.0, max_range=np.inf, terms=False):
    """-> dict(H [6, 6], g [6], cost, n_corr, n_points, and `abs_H`, `abs_g`, `abs_cost`: the sums of the absolute values of the
    terms of every entry -- what a bound on the rounding of another summation order is stated in).  terms: also the per-pair
    `r` [P, 3], `M` [P, 3, 3] and `q` [P, 3]."""
    X = np.asarray(X, np.float64)
    w, cells = world_points(table, cloud, X, min_range, max_range)
    i, row = pairs(table, cells, min_points, neighbors)
    n = table.map.counts[row].astype(np.float64)
    mu = table.map.sums[row, :3].astype(np.float64) / n[:, None] / SCALE * np.float64(table.voxel)
    Sigma = MR.full(MR.covariance(table.sums[row], table.map.counts[row], table.voxel)) + np.float64(sigma) ** 2 * np.eye(3)
    M = np.linalg.inv(Sigma) if len(row) else np.zeros((0, 3, 3))
    r = w[i] - mu
    q = w[i] - X[:3, 3]
    J = np.concatenate([-skew(q), np.broadcast_to(np.eye(3), (len(row), 3, 3))], 2)  # [P, 3, 6]
    MJ = M @ J
    Hk = np.swapaxes(J, 1, 2) @ MJ                      # [P, 6, 6]
    Mr = (M @ r[:, :, None])[:, :, 0]
    gk = (np.swapaxes(J, 1, 2) @ Mr[:, :, None])[:, :, 0]  # [P, 6]
    ck = (r * Mr).sum(1)
    out = dict(H=Hk.sum(0), g=gk.sum(0), cost=float(ck.sum()), n_corr=len(row), n_points=len(w),
               abs_H=np.abs(Hk).sum(0), abs_g=np.abs(gk).sum(0), abs_cost=float(np.abs(ck).sum()))
    return dict(out, r=r, M=M, q=q) if terms else out


def cholesky_solve(H, g):
    """delta with H delta = -g by H = L L^T without pivoting, or None if a pivot is <= 0 or not finite."""
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0.0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
    delta = np.zeros(6)
    for i in range(5, -1, -1):
        delta[i] = (y[i] - L[i + 1:, i] @ delta[i + 1:]) / L[i, i]
    return delta


def apply(X, delta):
    """R <- Exp(omega) R, t <- t + v."""
    out = np.array(X, np.float64, copy=True)
    out[:3, :3] = exp_so3(delta[:3]) @ out[:3, :3]
    out[:3, 3] = out[:3, 3] + delta[3:]
    return out


def register(table, cloud, X0, sigma=0.02, min_points=4, neighbors=1, max_iteration=30, rot_eps=1e-5, trans_eps=1e-4, min_range=0.0,
             max_range=np.inf):
    """-> dict(transform [4, 4], H, g, cost, abs_*, n_corr, n_points, iterations, status)."""
    X = np.array(X0, np.float64, copy=True)
    updates, last = 0, False
    while True:
        e = evaluate(table, cloud, X, sigma, min_points, neighbors, min_range, max_range)
        status = None
        if last:
            status = 1
        elif updates >= max_iteration:
            status = 0
        else:
            delta = cholesky_solve(e['H'], e['g']) if e['n_corr'] > 0 else None
            if delta is None:
                status = 2
        if status is not None:
            return dict(e, transform=X, iterations=updates, status=status)
        X = apply(X, delta)
        updates += 1
        last = bool(np.linalg.norm(delta[:3]) < rot_eps and np.linalg.norm(delta[3:]) < trans_eps)
