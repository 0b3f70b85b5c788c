"""Float64 numpy restatement of what rdm_eval_pairs computes per pair (experiments/eval.py:100-239 of the reference):
the --num_corr selection, the weighted Procrustes of method svd, the fine meters, the coarse precision and the registration
error.  Everything is float64 on the stored fp32 values, so a threshold decision can differ from an fp32 evaluation only for
rows within rounding distance of the threshold: `fine` reports those as `undecided` counts (relative margin 1e-5)."""
import math

import numpy as np

MARGIN = 1e-5  # relative distance to a radius below which a row's side of it is left open
FIELDS = ('num_corr', 'residual', 'inlier_ratio', 'inlier_ratio_0.3', 'inlier_ratio_0.1', 'overlap', 'precision', 'rre', 'rte',
          'rx', 'ry', 'rz')


def select(scores, num_corr):
    """eval.py:121-125 with the open order fixed: the first num_corr rows in (score descending, row ascending), returned in
    row order; every row when num_corr is None or C <= num_corr."""
    c = len(scores)
    if num_corr is None or c <= num_corr:
        return np.arange(c)
    order = np.lexsort((np.arange(c), -np.asarray(scores, np.float64)))[:num_corr]
    return np.sort(order)


def weighted_procrustes(src, ref, scores, eps=1e-5):
    """procrustes.py:6-73 (weight_thresh 0) in float64 -> 4x4."""
    src, ref = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    w = np.asarray(scores, np.float64).copy()
    w[w < 0] = 0
    w = w / (w.sum() + eps)
    cs, cr = (src * w[:, None]).sum(0), (ref * w[:, None]).sum(0)
    h = (src - cs).T @ (w[:, None] * (ref - cr))
    u, _, vt = np.linalg.svd(h)
    v = vt.T
    d = np.eye(3)
    d[2, 2] = np.sign(np.linalg.det(v @ u.T)) if np.abs(h).sum() > 0 else 1.0
    r = v @ d @ u.T if np.abs(h).sum() > 0 else np.eye(3)
    t = np.eye(4)
    t[:3, :3] = r
    t[:3, 3] = cr - r @ cs
    return t


def singular_ratio(src, ref, scores, eps=1e-5):
    """sigma_2 / sigma_1 of the covariance weighted_procrustes decomposes (rank test of the svd cases)."""
    src, ref = np.asarray(src, np.float64), np.asarray(ref, np.float64)
    w = np.asarray(scores, np.float64) / (np.asarray(scores, np.float64).sum() + eps)
    cs, cr = (src * w[:, None]).sum(0), (ref * w[:, None]).sum(0)
    s = np.linalg.svd((src - cs).T @ (w[:, None] * (ref - cr)), compute_uv=False)
    return s[1] / s[0]


def nearest_distances(q, s):
    """Exact nearest-neighbour distances, brute force in blocks (float64)."""
    out = np.empty(len(q))
    for i in range(0, len(q), 512):
        d = q[i:i + 512, None, :] - s[None, :, :]
        out[i:i + 512] = np.sqrt((d * d).sum(2).min(1))
    return out


def fine(ref, src, gt_transform, radius):
    """registration.py:175-200,361-375 in float64.  -> dict: num_corr, residual, and per threshold name the count of rows
    decidedly below it (`lo`) and the count within MARGIN of it (`undecided`): a correct fp32 evaluation counts between lo and
    lo + undecided rows."""
    ref, src = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(src, np.float64).reshape(-1, 3)
    t = np.asarray(gt_transform, np.float64)
    n = len(ref)
    out = {'num_corr': n}
    if n == 0:
        out['residual'] = float('nan')
        for name in ('inlier_ratio', 'inlier_ratio_0.3', 'inlier_ratio_0.1', 'overlap'):
            out[name] = {'lo': 0, 'undecided': 0}
        return out
    moved = src @ t[:3, :3].T + t[:3, 3]
    res = np.sqrt(((ref - moved) ** 2).sum(1))
    out['residual'] = float(res.mean())
    for name, r in (('inlier_ratio', radius), ('inlier_ratio_0.3', 0.3), ('inlier_ratio_0.1', 0.1)):
        open_ = np.abs(res - r) <= MARGIN * r
        out[name] = {'lo': int(((res < r) & ~open_).sum()), 'undecided': int(open_.sum())}
    nn = nearest_distances(ref, moved)
    open_ = np.abs(nn - radius) <= MARGIN * radius
    out['overlap'] = {'lo': int(((nn < radius) & ~open_).sum()), 'undecided': int(open_.sum())}
    return out


def coarse(node_dims, ref_idx, src_idx, gt_idx):
    """registration.py:378-402: -> (hit cells, predicted cells, ground-truth cells, precision), cells counted once."""
    n = int(node_dims[1])
    pred = {int(r) * n + int(s) for r, s in zip(ref_idx, src_idx)}
    gt = {int(r) * n + int(s) for r, s in np.asarray(gt_idx).reshape(-1, 2)}
    hit = len(pred & gt)
    return hit, len(pred), len(gt), hit / (len(pred) + 1e-12)


def euler_degrees(r):
    sy = math.sqrt(r[0, 0] * r[0, 0] + r[1, 0] * r[1, 0])
    if sy >= 1e-6:
        x, y, z = math.atan2(r[2, 1], r[2, 2]), math.atan2(-r[2, 0], sy), math.atan2(r[1, 0], r[0, 0])
    else:
        x, y, z = math.atan2(-r[1, 2], r[1, 1]), math.atan2(-r[2, 0], sy), 0
    return tuple(v * 180.0 / 3.141592653589793 for v in (x, y, z))


def registration_error(gt_transform, est_transform):
    """registration.py:17-108 on float64 copies -> (rre degrees, rte, |d roll|, |d pitch|, |d yaw|)."""
    g, e = np.asarray(gt_transform, np.float64), np.asarray(est_transform, np.float64)
    x = 0.5 * (np.trace(e[:3, :3].T @ g[:3, :3]) - 1.0)
    rre = 180.0 * np.arccos(np.clip(x, -1.0, 1.0)) / np.pi
    rte = np.linalg.norm(g[:3, 3] - e[:3, 3])
    a, b = euler_degrees(g[:3, :3]), euler_degrees(e[:3, :3])
    return float(rre), float(rte), abs(a[0] - b[0]), abs(a[1] - b[1]), abs(a[2] - b[2])


def evaluate(pair, method='lgr', num_corr=None, radius=0.6, est_transform=None):
    """One pair dict (the arrays of a pair file, `node_dims` or ref/src_points_c) -> dict: `rows` (the selection), `fine`,
    `coarse`, `transform` (float64 4x4: stored, Procrustes, or `est_transform` when given -- method ransac) and
    `registration`."""
    rows = select(pair['corr_scores'], num_corr)
    ref, src, sc = pair['ref_corr_points'][rows], pair['src_corr_points'][rows], pair['corr_scores'][rows]
    dims = pair['node_dims'] if 'node_dims' in pair else (len(pair['ref_points_c']), len(pair['src_points_c']))
    if est_transform is not None:
        t = np.asarray(est_transform, np.float64)
    elif method == 'lgr':
        t = np.asarray(pair['estimated_transform'], np.float64)
    elif method == 'svd':
        t = weighted_procrustes(src, ref, sc)
    else:
        raise ValueError(method)
    return {'rows': rows, 'fine': fine(ref, src, pair['transform'], radius),
            'coarse': coarse(dims, pair['ref_node_corr_indices'], pair['src_node_corr_indices'], pair['gt_node_corr_indices']),
            'transform': t, 'registration': registration_error(pair['transform'], t)}
