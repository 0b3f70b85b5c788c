"""Float64 restatement of rdm_information_matrix (rdmnet_amd/csrc/nearest.hip): Open3D's published arithmetic of
get_information_matrix_from_point_clouds and evaluate_registration, with this library's definitions where Open3D leaves them
library-internal (Open3D is not installed and not part of the reference tree: parity unpinned).
  The search is tests/nearest_restatement.py's: fp32 points read as double, an optional float64 4x4 transform per cloud,
  x' = ((R00 x + R01 y) + R02 z) + t0, d2 = ((dx dx) + (dy dy)) + (dz dz), the LOWEST target row among equal distances.
  Source row i has the correspondence (i, j) iff sqrt(d2[i]) < r (strict), j its nearest target row.
  With p = (x, y, z) the MOVED target point of a correspondence, the matrix is the sum of g g^T over the three rows
  (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1) -- rotation first, then translation -- added literally here: every
  entry is the math.fsum (the exactly rounded sum) of its 3 C products, each product rounded once in double.
`closed_form` is the kernel's route to the same matrix (C, sum p, sum p p^T); tests/test_information.py holds the two together."""
import math

import numpy as np

import nearest_restatement as R


def correspondences(source, target, radius, s_transform=None, t_transform=None):
    """-> (corr int64 [C, 2] rows (i, j) in ascending i, d2 float64 [C], the moved target points float64 [n_t, 3])."""
    d2, idx = R.nearest(source, target, s_transform, t_transform)
    rows = np.nonzero(np.sqrt(d2) < np.float64(radius))[0]
    return np.stack([rows, idx[rows]], axis=1).astype(np.int64).reshape(-1, 2), d2[rows], R.moved(target, t_transform)


def jacobian_rows(p):
    x, y, z = (float(v) for v in p)
    return ((0.0, z, -y, 1.0, 0.0, 0.0), (-z, 0.0, x, 0.0, 1.0, 0.0), (y, -x, 0.0, 0.0, 0.0, 1.0))


def row_form(points):
    """points: the moved target point of every correspondence [C, 3] -> (the matrix float64 [6, 6], every entry the fsum of its
    terms; magnitude float64 [6, 6], the fsum of the terms' absolute values: what a rounding bound of the entry scales with)."""
    terms = [[[] for _ in range(6)] for _ in range(6)]
    for p in np.asarray(points, np.float64).reshape(-1, 3):
        for g in jacobian_rows(p):
            for a in range(6):
                for b in range(6):
                    terms[a][b].append(g[a] * g[b])
    info = np.array([[math.fsum(t) for t in row] for row in terms], np.float64).reshape(6, 6)
    magnitude = np.array([[math.fsum(abs(v) for v in t) for t in row] for row in terms], np.float64).reshape(6, 6)
    return info + 0.0, magnitude


def closed_form(points):
    """The same matrix from C = sum 1, s = sum p and M = sum p p^T: rotation block tr(M) I - M, translation block C I, upper-right
    block [s]x, its transpose below.  The diagonal of the rotation block is formed as Myy + Mzz, Mxx + Mzz, Mxx + Myy, as the kernel
    forms it: tr(M) - Mxx would round at the size of Mxx, which is no term of that entry."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    c, s = float(p.shape[0]), [math.fsum(p[:, a]) for a in range(3)]
    M = np.array([[math.fsum(p[:, a] * p[:, b]) for b in range(3)] for a in range(3)], np.float64).reshape(3, 3)
    cross = np.array([[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]])
    info = np.zeros((6, 6))
    info[:3, :3] = np.diag([M[1, 1] + M[2, 2], M[0, 0] + M[2, 2], M[0, 0] + M[1, 1]]) - (M - np.diag(np.diag(M)))
    info[:3, 3:] = cross
    info[3:, :3] = cross.T
    info[3:, 3:] = c * np.eye(3)
    return info + 0.0


def information(source, target, radius, s_transform=None, t_transform=None):
    """-> dict(information [6, 6], magnitude [6, 6], corr int64 [C, 2], C, sum_d2 (fsum), fitness, inlier_rmse)."""
    corr, d2, moved_target = correspondences(source, target, radius, s_transform, t_transform)
    info, magnitude = row_form(moved_target[corr[:, 1]])
    c, n = int(corr.shape[0]), np.asarray(source).shape[0]
    sum_d2 = math.fsum(d2)
    return {'information': info, 'magnitude': magnitude, 'corr': corr, 'C': c, 'sum_d2': sum_d2, 'fitness': c / n if n > 0 else 0.0,
            'inlier_rmse': math.sqrt(sum_d2 / c) if c > 0 else 0.0}


def assert_decided(source, target, radius, s_transform=None, t_transform=None, boundary_rows=(), tie_rows=()):
    """Every row is decided: no nearest distance within 1e-9 relative of the radius (but the constructed boundary rows), and
    nearest and second nearest differ (but in the constructed tie rows)."""
    q, s = R.moved(source, s_transform), R.moved(target, t_transform)
    if q.shape[0] == 0 or s.shape[0] == 0:
        return
    d = np.sqrt(R.sq_dists(q, s))
    first = np.sort(d, axis=1)[:, :2]
    free = np.ones(q.shape[0], bool)
    free[list(boundary_rows)] = False
    assert (np.abs(first[free, 0] - radius) > 1e-9 * radius).all(), 'a nearest distance lies on the radius'
    if s.shape[0] > 1:
        free = np.ones(q.shape[0], bool)
        free[list(tie_rows)] = False
        assert (first[free, 1] > first[free, 0]).all(), 'nearest and second nearest are equal'
