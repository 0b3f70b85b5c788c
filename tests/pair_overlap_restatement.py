"""Float64 restatement of rdmnet_amd/csrc/ball_query.hip: get_correspondences and compute_overlap
(geotransformer/utils/registration.py:191-216) by blocked brute force, with the library's arithmetic:
  points are fp32 read as double, the transform a float64 4x4 (None leaves src as it is);
  x' = ((R00 x + R01 y) + R02 z) + t0 per row;  d = ref - src';  d2 = ((dx dx) + (dy dy)) + (dz dz);  r2 = r r in double;
  (i, j) is a correspondence iff d2 <= r2 (cKDTree's ball is closed), listed in ascending (i, j);
  a row overlaps iff sqrt(its smallest d2) < r (compute_overlap's comparison is strict).
numpy evaluates every expression below element-wise in double, one rounding per operation and never contracted."""
import numpy as np

BLOCK = 64  # ref rows per block (the block's temporaries stay in the cache)


def moved(src_points, transform):
    s = np.asarray(src_points)[:, :3].astype(np.float64)
    if transform is None:
        return s
    T = np.asarray(transform, dtype=np.float64)
    assert T.shape == (4, 4)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def sq_dists(ref_block, src_moved):
    """[B, M] float64: d2 of every (ref row, moved src row)."""
    r = np.asarray(ref_block)[:, :3].astype(np.float64)
    out = None
    for a in range(3):  # ((dx dx) + (dy dy)) + (dz dz), in place
        d = r[:, None, a] - src_moved[None, :, a]
        np.multiply(d, d, out=d)
        out = d if out is None else np.add(out, d, out=out)
    return out


def ball_query(ref_points, src_points, transform, radius):
    """-> dict(corr int64 [C, 2] ascending (i, j), d2 float64 [C] of those pairs, counts int64 [N], ref_min_d2 / src_min_d2
    float64 [N] / [M] (the smallest d2 over ALL rows of the other cloud, inf when that cloud is empty))."""
    ref_points, s = np.asarray(ref_points), moved(src_points, transform)
    n, m = ref_points.shape[0], s.shape[0]
    r2 = np.float64(radius) * np.float64(radius)
    rows, dists, counts = [], [], np.zeros((n,), np.int64)
    ref_min, src_min = np.full((n,), np.inf), np.full((m,), np.inf)
    for i0 in range(0, n, BLOCK):
        d2 = sq_dists(ref_points[i0:i0 + BLOCK], s)
        if m > 0:
            ref_min[i0:i0 + BLOCK] = d2.min(axis=1)
            src_min = np.minimum(src_min, d2.min(axis=0))
        hit = d2 <= r2
        i, j = np.nonzero(hit)  # row-major: ascending (i, j)
        rows.append(np.stack([i + i0, j], axis=1).astype(np.int64))
        dists.append(d2[i, j])
        counts[i0:i0 + BLOCK] = hit.sum(axis=1)
    corr = np.concatenate(rows, axis=0) if rows else np.zeros((0, 2), np.int64)
    return dict(corr=corr.reshape(-1, 2), d2=np.concatenate(dists) if dists else np.zeros((0,)), counts=counts, ref_min_d2=ref_min,
                src_min_d2=src_min)


def narrowed(q, radius):
    """ball_query's result at a smaller radius, from the pairs of the larger one (the minima do not depend on the radius)."""
    keep = q['d2'] <= np.float64(radius) * np.float64(radius)
    corr = q['corr'][keep]
    return dict(q, corr=corr, d2=q['d2'][keep], counts=np.bincount(corr[:, 0], minlength=len(q['counts'])).astype(np.int64))


def get_correspondences(ref_points, src_points, transform=None, matching_radius=None):
    return ball_query(ref_points, src_points, transform, matching_radius)['corr']


def _fraction(min_d2, radius):
    return float(np.mean(np.sqrt(min_d2) < np.float64(radius))) if len(min_d2) else 0.0


def compute_overlap(ref_points, src_points, transform=None, positive_radius=0.1, both=False):
    q = ball_query(ref_points, src_points, transform, positive_radius)
    o_ref, o_src = _fraction(q['ref_min_d2'], positive_radius), _fraction(q['src_min_d2'], positive_radius)
    return (o_ref, o_src) if both else o_ref


def overlap_labels(ref_points, src_points, transform, radius):
    corr = get_correspondences(ref_points, src_points, transform, radius)
    n, m = np.asarray(ref_points).shape[0], np.asarray(src_points).shape[0]
    return np.isin(np.arange(n), corr[:, 0]), np.isin(np.arange(m), corr[:, 1])
