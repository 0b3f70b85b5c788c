"""Float64 restatement of rdmnet_amd/csrc/nearest.hip: get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22) and what
the reference builds on it (geotransformer/utils/registration.py:136-197) by blocked brute force, with the library's arithmetic:
  points are fp32 read as double, each cloud has an optional float64 4x4 transform (None leaves it as it is);
  x' = ((R00 x + R01 y) + R02 z) + t0 per row;  d = q' - s';  d2 = ((dx dx) + (dy dy)) + (dz dz);
  d2[i] = the smallest d2 over all support rows, idx[i] = the LOWEST support row that attains it (np.argmin returns the first);
  the distance is sqrt(d2);  an empty support cloud gives inf and index n_s.
numpy evaluates every expression below element-wise in double, one rounding per operation and never contracted.  The sums of
the scalar measures are numpy's (pairwise): the library's fixed order differs from them by round-off only, which the tests bound."""
import numpy as np

BLOCK = 64  # query rows per block (the block's temporaries stay in the cache)


def moved(points, transform):
    p = np.asarray(points)[:, :3].astype(np.float64)
    if transform is None:
        return p
    T = np.asarray(transform, dtype=np.float64)
    assert T.shape == (4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def sq_dists(q_block, s_moved):
    """[B, M] float64: d2 of every (moved query row, moved support row)."""
    out = None
    for a in range(3):  # ((dx dx) + (dy dy)) + (dz dz), in place
        d = q_block[:, None, a] - s_moved[None, :, a]
        np.multiply(d, d, out=d)
        out = d if out is None else np.add(out, d, out=out)
    return out


def nearest(q_points, s_points, q_transform=None, s_transform=None):
    """-> (d2 float64 [n_q], idx int64 [n_q])."""
    q, s = moved(q_points, q_transform), moved(s_points, s_transform)
    n, m = q.shape[0], s.shape[0]
    d2, idx = np.full((n,), np.inf), np.full((n,), m, np.int64)
    if m > 0:
        for i0 in range(0, n, BLOCK):
            d = sq_dists(q[i0:i0 + BLOCK], s)
            j = np.argmin(d, axis=1)  # the first among equal values
            idx[i0:i0 + BLOCK] = j
            d2[i0:i0 + BLOCK] = d[np.arange(d.shape[0]), j]
    return d2, idx


def get_nearest_neighbor(q_points, s_points, return_index=False, q_transform=None, s_transform=None):
    d2, idx = nearest(q_points, s_points, q_transform, s_transform)
    return (np.sqrt(d2), idx) if return_index else np.sqrt(d2)


def compute_overlap(ref_points, src_points, transform=None, positive_radius=0.1):
    return float(np.mean(get_nearest_neighbor(ref_points, src_points, s_transform=transform) < positive_radius))


def compute_modified_chamfer_distance(raw_points, ref_points, src_points, gt_transform, est_transform):
    gt, est = np.asarray(gt_transform, np.float64), np.asarray(est_transform, np.float64)
    p_q = get_nearest_neighbor(src_points, raw_points, q_transform=est).mean()
    q_p = get_nearest_neighbor(ref_points, raw_points, s_transform=np.matmul(est, np.linalg.inv(gt))).mean()
    return float(p_q + q_p)


def compute_registration_rmse(src_points, gt_transform, est_transform):
    d = moved(src_points, gt_transform) - moved(src_points, est_transform)
    return float(np.sqrt(((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])).mean())


def side_totals(q_points, s_points, q_transform, s_transform, radius):
    """(rows with sqrt(d2) < radius (strict), their sum of d2, the sum of all nearest distances)."""
    d2, _ = nearest(q_points, s_points, q_transform, s_transform)
    near = np.sqrt(d2) < np.float64(radius)
    return int(near.sum()), float(d2[near].sum()), float(np.sqrt(d2).sum())


def alignment_quality(ref_points, src_points, transform, radius):
    out = {}
    n_ref, n_src = np.asarray(ref_points).shape[0], np.asarray(src_points).shape[0]
    sides = (('ref', n_ref, side_totals(ref_points, src_points, None, transform, radius)),
             ('src', n_src, side_totals(src_points, ref_points, transform, None, radius)))
    chamfer = 0.0
    for side, n, (within, sum_d2, sum_dist) in sides:
        out[f'fitness_{side}'] = within / n if n > 0 else 0.0
        out[f'inlier_rmse_{side}'] = float(np.sqrt(sum_d2 / within)) if within > 0 else 0.0
        out[f'n_within_{side}'] = within
        chamfer += sum_dist / n if n > 0 else float('nan')
    out['chamfer'] = chamfer
    out['n_ref'], out['n_src'] = n_ref, n_src
    return out
