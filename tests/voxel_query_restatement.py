"""NumPy restatement (float64) of the per-point queries of the voxel map (include/rdmnet_hip.h, "voxel map queries"; DESIGN.md section
7), written from the definition on top of the other restatements and sharing no code with the library.  The map is a
voxel_moments_restatement.Moments (sorted keys, counts, the C sums, the nine moment sums) and, for the observations, a
voxel_observations_restatement.Observed of the same scans: both sort their voxels by key, so their rows are the same voxels.

Per row of a scan at the pose X:
  gate      as the map's integrate: a non-finite value among its C -> NONFINITE, else outside the range -> RANGE, else a cell outside
            [-2^20, 2^20) or an attribute of 2^20 or more -> EXTENT (voxel_register_restatement.world_points keeps the others);
  visit     cell + o, o = 0 ... neighbors - 1, in the registration's order; a voxel takes part if it is in the map with at least
            min_points points (voxel_register_restatement.pairs);
  per voxel r = w - mu, Sigma = cov + sigma^2 I (cov = 0 without moments), M = Sigma^-1 (numpy.linalg.inv), d2_o = the sum of the nine
            terms r_a M_ab r_b;
  best      the smallest d2_o, the smallest o on a tie;
  label     no voxel -> UNMAPPED; the best voxel's scans < min_scans -> TRANSIENT; d2 > max_d2 -> OFF_SURFACE; else STATIC."""
import numpy as np

import voxel_map_restatement as VM
import voxel_moments_restatement as MR
import voxel_observations_restatement as OR
import voxel_register_restatement as RR

NONFINITE, RANGE, EXTENT, UNMAPPED, TRANSIENT, OFF_SURFACE, STATIC = range(7)
LABELS = ('nonfinite', 'range', 'extent', 'unmapped', 'transient', 'off_surface', 'static')
INTEGERS = ('labels', 'best', 'counts', 'scans', 'first', 'last', 'pairs')


def gates(cloud, X, voxel, channels, min_range=0.0, max_range=np.inf):
    """-> the label 0, 1 or 2 of every row that a gate stops, -1 for the rows that pass."""
    p = np.asarray(cloud, np.float32)[:, :channels].astype(np.float64)
    X = np.asarray(X, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        finite = np.isfinite(p).all(1)
        r2 = (x * x + y * y) + z * z
        in_range = (np.float64(min_range) * np.float64(min_range) <= r2) & (r2 <= np.float64(max_range) * np.float64(max_range))
        w = np.stack([((X[d, 0] * x + X[d, 1] * y) + X[d, 2] * z) + X[d, 3] for d in range(3)], 1)
        f = np.floor(w / np.float64(voxel) * VM.SCALE)
        inside = ((f >= -2.0 ** 40) & (f < 2.0 ** 40)).all(1) & (np.abs(p[:, 3:]) < VM.SCALE).all(1)
    return np.where(~finite, NONFINITE, np.where(~in_range, RANGE, np.where(~inside, EXTENT, -1)))


def query(table, observed, cloud, X, sigma=0.02, min_points=1, neighbors=1, min_scans=1, max_d2=np.inf, min_range=0.0,
          max_range=np.inf, moments=True):
    """One scan -> dict of arrays with one row per row of `cloud`: labels, best, counts, scans, first, last, d2, d2_sum, pairs (the
    library's outputs), `each` [N, 7] (d2_o, inf where voxel o did not take part) and `abs_d2`, `abs_sum`: the sums of the absolute
    values of the terms r_a M_ab r_b of d2 and of d2_sum -- what a bound on the rounding of another order of operations is stated
    in.  observed None: a map without observations (min_scans <= 1)."""
    assert observed is not None or min_scans <= 1
    if observed is not None:
        assert np.array_equal(observed.map.keys, table.keys)
    N = len(cloud)
    gate = gates(cloud, X, table.voxel, table.map.channels, min_range, max_range)
    rows = np.nonzero(gate < 0)[0]
    w, cells = RR.world_points(table, cloud, X, min_range, max_range)
    assert len(w) == len(rows), 'the gates here and in voxel_register_restatement.world_points differ'
    i, row = RR.pairs(table, cells, min_points, neighbors)
    # which offset a pair belongs to: pairs are ordered by point and then by offset, and `row` names the voxel
    key = table.keys[row] if len(row) else np.zeros(0, np.uint64)
    vc = np.stack([((key >> np.uint64(42)) & np.uint64(0x1fffff)).astype(np.int64) - VM.HALF,
                   ((key >> np.uint64(21)) & np.uint64(0x1fffff)).astype(np.int64) - VM.HALF,
                   (key & np.uint64(0x1fffff)).astype(np.int64) - VM.HALF], 1) if len(row) else np.zeros((0, 3), np.int64)
    delta = vc - cells[i]
    same = (delta[:, None, :] == RR.OFFSETS[None]).all(2)
    assert same.sum(1).tolist() == [1] * len(row)
    o = np.argmax(same, 1)
    n = table.map.counts[row].astype(np.float64)
    mu = table.map.sums[row, :3].astype(np.float64) / n[:, None] / VM.SCALE * np.float64(table.voxel)
    cov = MR.full(MR.covariance(table.sums[row], table.map.counts[row], table.voxel)) if moments else np.zeros((len(row), 3, 3))
    M = np.linalg.inv(cov + np.float64(sigma) ** 2 * np.eye(3)) if len(row) else np.zeros((0, 3, 3))
    r = w[i] - mu
    terms = r[:, :, None] * M * r[:, None, :]  # [P, 3, 3]
    d2o, a2o = terms.sum((1, 2)), np.abs(terms).sum((1, 2))
    each = np.full((len(rows), 7), np.inf)
    each_abs = np.zeros((len(rows), 7))
    each_row = np.full((len(rows), 7), -1, np.int64)
    each[i, o], each_abs[i, o], each_row[i, o] = d2o, a2o, row
    took = each_row >= 0
    best = np.where(took.any(1), np.argmin(each, 1), -1)  # (the first minimum: the smallest o)
    pick = np.arange(len(rows)), np.maximum(best, 0)
    has = best >= 0
    best_row = np.where(has, each_row[pick], 0)
    out = dict(labels=np.zeros(N, np.uint8), best=np.full(N, -1, np.int8), counts=np.zeros(N, np.int32), scans=np.zeros(N, np.int32),
               first=np.full(N, OR.MAX_ID, np.int32), last=np.full(N, -1, np.int32), d2=np.full(N, np.inf), d2_sum=np.zeros(N),
               pairs=np.zeros(N, np.uint8), each=np.full((N, 7), np.inf), abs_d2=np.zeros(N), abs_sum=np.zeros(N))
    out['labels'][gate >= 0] = gate[gate >= 0]
    out['best'][rows] = best
    out['pairs'][rows] = took.sum(1)
    out['each'][rows] = each
    out['d2'][rows] = np.where(has, each[pick], np.inf)
    out['abs_d2'][rows] = np.where(has, each_abs[pick], 0.0)
    total = np.zeros(len(rows))
    for k in range(7):  # ascending o, as the library adds them
        total = total + np.where(took[:, k], each[:, k], 0.0)
    out['d2_sum'][rows] = total
    out['abs_sum'][rows] = each_abs.sum(1)
    if len(table.keys):
        out['counts'][rows] = np.where(has, table.map.counts[best_row], 0)
    label = np.full(len(rows), STATIC, np.uint8)
    if observed is not None and len(table.keys):
        for name, none in (('scans', 0), ('first', OR.MAX_ID), ('last', -1)):
            out[name][rows] = np.where(has, getattr(observed, name)[best_row], none)
        label[out['scans'][rows] < min_scans] = TRANSIENT
    with np.errstate(invalid='ignore'):
        off = has & (out['d2'][rows] > np.float64(max_d2)) & (label == STATIC)
    label[off] = OFF_SURFACE
    label[~has] = UNMAPPED
    out['labels'][rows] = label
    return out


def batch(table, observed, clouds, poses, **kw):
    """The scans of a batch -> query's dict with the rows of all scans one after the other, `offsets` int64 [n + 1] and `tallies` int64
    [n, 8]: per scan the rows of each label, then the sum of `pairs`."""
    parts = [query(table, observed, c, X, **kw) for c, X in zip(clouds, poses)]
    names = list(parts[0]) if parts else []
    out = {k: np.concatenate([p[k] for p in parts]) for k in names}
    out['offsets'] = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    out['tallies'] = np.array([[int((p['labels'] == k).sum()) for k in range(7)] + [int(p['pairs'].sum(dtype=np.int64))] for p in parts],
                              np.int64).reshape(-1, 8)
    return out
