"""NumPy restatement (float64) of the map-to-map alignment on the per-voxel Gaussians of both sides (include/rdmnet_hip.h, "voxel map
alignment"), written from the definition and sharing no code with the library.  Target and source are
voxel_moments_restatement.Moments maps: sorted keys, counts, the C sums and the nine moment sums; their voxel sizes may differ.

One evaluation of a source at the pose X = (R, t) (target <- source):
  gate      a source voxel with fewer than source_min_points points is passed over and counted nowhere;
  source    mu_b = (sum / n) / 2^20 source_voxel, Sigma_b = the moments' covariance with source_voxel;
  transform w_d = ((R[d,0] mu_x + R[d,1] mu_y) + R[d,2] mu_z) + t_d, Q_d = floor(w_d / voxel 2^20), cell_d = Q_d >> 20 on the target's
            grid; a record the target would count in out_of_extent is dropped, the others are `n_points`;
  visit     the 1 or 7 cells of the registration, under its rule (in the target with n >= min_points);
  per pair  mu_a, Sigma_a of the target voxel; C = (R Sigma_b) R^T, every entry as ((x0 + x1) + x2); M = (Sigma_a + C + sigma^2 I)^-1
            (numpy.linalg.inv), r = w - mu_a, q = w - t, J = [-[q]x | I3];
  totals    H = sum J^T M J, g = sum J^T M r, cost = sum r^T M r, n_corr = the number of pairs; every pair has weight one.
M is held fixed in the linearisation.  The iteration is the registration's."""
import numpy as np

import voxel_moments_restatement as MR
from voxel_register_restatement import apply, cholesky_solve, pairs, skew

SCALE = 1048576.0


def source_gaussians(source, source_min_points):
    """-> (mu float64 [K, 3], Sigma_b [K, 3, 3]) of the source voxels with at least source_min_points points, in key order."""
    take = source.map.counts >= int(source_min_points)
    n = source.map.counts[take].astype(np.float64)
    mu = source.map.sums[take, :3].astype(np.float64) / n[:, None] / SCALE * np.float64(source.voxel)
    return mu, MR.full(MR.covariance(source.sums[take], source.map.counts[take], source.voxel))


def world_means(target, mu, Sb, X):
    """The transform and the extent gate on the target's grid -> (w [K', 3], cells int64 [K', 3], Sigma_b [K', 3, 3])."""
    voxel = np.float64(target.voxel)
    x, y, z = mu[:, 0], mu[:, 1], mu[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.stack([((X[d, 0] * x + X[d, 1] * y) + X[d, 2] * z) + X[d, 3] for d in range(3)], 1)
        f = np.floor(w / voxel * SCALE)
        keep = ((f >= -2.0 ** 40) & (f < 2.0 ** 40)).all(1)
    return w[keep], f[keep].astype(np.int64) >> 20, Sb[keep]


def rotated(R, Sb):
    """C = (R Sigma_b) R^T [K, 3, 3] with the definition's association (symmetric: the lower entries are the upper's)."""
    P = np.stack([np.stack([(R[a, 0] * Sb[:, 0, b] + R[a, 1] * Sb[:, 1, b]) + R[a, 2] * Sb[:, 2, b] for b in range(3)], 1) for a in range(3)], 1)
    C = np.zeros_like(Sb)
    for a in range(3):
        for b in range(a, 3):
            C[:, a, b] = C[:, b, a] = (P[:, a, 0] * R[b, 0] + P[:, a, 1] * R[b, 1]) + P[:, a, 2] * R[b, 2]
    return C


def evaluate(target, source, X, sigma=0.02, min_points=4, source_min_points=4, neighbors=7):
    """-> dict(H [6, 6], g [6], cost, n_corr, n_points, and `abs_H`, `abs_g`, `abs_cost`: the sums of the absolute values of the
    terms of every entry)."""
    X = np.asarray(X, np.float64)
    mu, Sb = source_gaussians(source, source_min_points)
    w, cells, Sb = world_means(target, mu, Sb, X)
    i, row = pairs(target, cells, min_points, neighbors)
    n = target.map.counts[row].astype(np.float64)
    mu_a = target.map.sums[row, :3].astype(np.float64) / n[:, None] / SCALE * np.float64(target.voxel)
    Sigma_a = MR.full(MR.covariance(target.sums[row], target.map.counts[row], target.voxel))
    C = rotated(X[:3, :3], Sb)
    Sigma = (Sigma_a + C[i]) + np.float64(sigma) ** 2 * np.eye(3)
    M = np.linalg.inv(Sigma) if len(row) else np.zeros((0, 3, 3))
    r = w[i] - mu_a
    q = w[i] - X[:3, 3]
    J = np.concatenate([-skew(q), np.broadcast_to(np.eye(3), (len(row), 3, 3))], 2)  # [P, 3, 6]
    Hk = np.swapaxes(J, 1, 2) @ (M @ J)
    Mr = (M @ r[:, :, None])[:, :, 0]
    gk = (np.swapaxes(J, 1, 2) @ Mr[:, :, None])[:, :, 0]
    ck = (r * Mr).sum(1)
    return dict(H=Hk.sum(0), g=gk.sum(0), cost=float(ck.sum()), n_corr=len(row), n_points=len(w),
                abs_H=np.abs(Hk).sum(0), abs_g=np.abs(gk).sum(0), abs_cost=float(np.abs(ck).sum()))


def align(target, source, X0, sigma=0.02, min_points=4, source_min_points=4, neighbors=7, max_iteration=30, rot_eps=1e-5, trans_eps=1e-4):
    """-> dict(transform [4, 4], H, g, cost, abs_*, n_corr, n_points, iterations, status)."""
    X = np.array(X0, np.float64, copy=True)
    updates, last = 0, False
    while True:
        e = evaluate(target, source, X, sigma, min_points, source_min_points, neighbors)
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
