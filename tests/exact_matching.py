"""Exact CPU restatements of the index kernels of matching.hip: NMS (a10), the point-to-node partition (a11) and the
superpoint matching with its global top-k (a12).

Every restatement follows the library's documented rules to the bit: the fp32 distance formula of common.h
(ref_sq_dist) through a correctly rounded fp32 fma, argmin keeping the first minimum, patches ordered by (distance bits,
point index), and the top-k ordered by (fp32 score descending, flat index ascending).  numpy only.
"""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ fma
def fma32(a, b, c):
    """Correctly rounded fp32 fmaf(a, b, c), elementwise (round to nearest even).

    a*b of two fp32 values is exact in fp64 (48 significant bits, exponent far inside fp64's range).  s = fl64(p + c)
    and its exact error e come from TwoSum.  Where e != 0 and s has an even last bit, s moves one ulp toward e: that is
    p + c rounded to odd at 53 bits, and rounding that to 24 bits is the correct rounding of p + c (53 >= 24 + 2)."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bv = s - p
    e = (p - (s - bv)) + (c - bv)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def ref_sq_dist(x, y):
    """common.h ref_sq_dist for every (x row, y row): [m, 3] x [n, 3] fp32 -> [m, n] fp32.
    xy = fma(x2, y2, fma(x1, y1, x0*y0)); |v|^2 = (v0*v0 + v1*v1) + v2*v2; d = (|x|^2 - 2*xy) + |y|^2, clamped at 1e-12."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    xn = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    yn = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
    X, Y = x[:, None, :], y[None, :, :]
    xy = fma32(X[..., 2], Y[..., 2], fma32(X[..., 1], Y[..., 1], X[..., 0] * Y[..., 0]))
    d = (xn[:, None] - F32(2) * xy) + yn[None, :]
    return np.maximum(d, F32(1e-12))


# ------------------------------------------------------------------------------------------------------------ NMS
def nms(idx, width=None):
    """rdmnet/vote/vote.py:13-40 over an explicit [n, h] index table: node i is kept iff none of its neighbours was kept
    before it.  Padding is index n; only the first `width` columns are read."""
    idx = np.asarray(idx, np.int64)
    n = idx.shape[0]
    if width is not None:
        idx = idx[:, :max(0, min(int(width), idx.shape[1]))]
    keep = np.zeros(n + 1, dtype=bool)
    rows = idx.tolist()
    for i in range(n):
        if not any(keep[j] for j in rows[i]):
            keep[i] = True
    return keep[:n]


def nms_lower_links_ok(idx, keep, width=None):
    """The kept set as a graph property of the lower-index links (i -> j < i) the table holds: no kept node links a kept
    node (independent), and every dropped node links a kept one (maximal).  Returns (independent, maximal)."""
    idx = np.asarray(idx, np.int64)
    if width is not None:
        idx = idx[:, :max(0, min(int(width), idx.shape[1]))]
    n = idx.shape[0]
    keep = np.asarray(keep, bool)
    lower = (idx >= 0) & (idx < np.arange(n)[:, None])
    k_ext = np.concatenate([keep, [False]])
    hit = (lower & k_ext[np.where(lower, idx, n)]).any(1)
    return bool(not hit[keep].any()), bool(hit[~keep].all())


# ------------------------------------------------------------------------------------------------ point-to-node
def partition(points, nodes, chunk=1 << 22):
    """owner i64[n] = the first node of minimal ref_sq_dist from each point, d_own f32[n] = that distance."""
    points, nodes = np.asarray(points, F32), np.asarray(nodes, F32)
    n, m = points.shape[0], nodes.shape[0]
    owner = np.empty(n, np.int64)
    d_own = np.empty(n, F32)
    step = max(1, chunk // max(m, 1))
    for p0 in range(0, n, step):
        d = ref_sq_dist(nodes, points[p0:p0 + step])
        a = d.argmin(0)                              # the first minimum
        owner[p0:p0 + step] = a
        d_own[p0:p0 + step] = d[a, np.arange(d.shape[1])]
    return owner, d_own


def point_to_node(points, nodes, k, cap=4096, parts=None):
    """modules/ops/pointcloud_partition.py:60-107 with the library's tie rules.  Returns
    (node_mask u8[m], knn_idx i64[m, k], knn_mask u8[m, k], status, counts): owner and distance from `partition` (or
    `parts`, its result for these clouds); a node's patch = its points ordered by (fp32 distance, index), the first k,
    padded with index n and mask 0; status = 1 iff a node owns more than `cap` points (its row is then unspecified)."""
    n, m = len(points), len(nodes)
    owner, d_own = partition(points, nodes) if parts is None else parts
    counts = np.bincount(owner, minlength=m)
    order = np.lexsort((np.arange(n), d_own, owner))  # by owner, then distance (positive: bit order), then index
    starts = np.concatenate([[0], np.cumsum(counts)])
    knn = np.full((m, k), n, np.int64)
    kmask = np.zeros((m, k), np.uint8)
    for j in np.flatnonzero(counts):
        t = min(k, int(counts[j]))
        knn[j, :t] = order[starts[j]:starts[j] + t]
        kmask[j, :t] = 1
    return (counts > 0).astype(np.uint8), knn, kmask, int((counts > cap).any()), counts


# --------------------------------------------------------------------------------------------- coarse matching
def _dot64(a, b):
    """a @ b.T in fp64 with equal rows giving equal results (BLAS may treat two copies of a row differently)."""
    ua, ia = np.unique(a, axis=0, return_inverse=True)
    ub, ib = np.unique(b, axis=0, return_inverse=True)
    return (ua.astype(np.float64) @ ub.astype(np.float64).T)[ia.reshape(-1)][:, ib.reshape(-1)]


def coarse_scores64(ref_f, src_f, ref_mask, src_mask, dual=True, sim=None):
    """oracle.forward.coarse_matching's formula in fp64 over the full [m, n] matrix, masked entries -1: the valid rows and
    columns are compacted, scored exp(-max(2 - 2xy, 1e-12)) and, with `dual`, normalised (s / rowsum) * (s / colsum).
    `sim` (optional, [m, n]) replaces the fp64 dot products, e.g. by the fp32 GEMM the fp32 path is given."""
    rm, cm = np.asarray(ref_mask, bool), np.asarray(src_mask, bool)
    m, n = rm.size, cm.size
    out = np.full((m, n), -1.0)
    ri, si = np.flatnonzero(rm), np.flatnonzero(cm)
    if ri.size == 0 or si.size == 0:
        return out
    xy = _dot64(np.asarray(ref_f, F32)[ri], np.asarray(src_f, F32)[si]) if sim is None else \
        np.asarray(sim, np.float64)[np.ix_(ri, si)]
    s = np.exp(-np.maximum(2.0 - 2.0 * xy, 1e-12))
    if dual:
        s = (s / s.sum(1, keepdims=True)) * (s / s.sum(0, keepdims=True))
    out[np.ix_(ri, si)] = s
    return out


def topk(scores32, k):
    """Global top-k of an fp32 [m, n] matrix over its entries >= 0, ordered by (score descending, flat index ascending)
    -> (row i64[c], col i64[c], score f32[c]), c = min(k, eligible entries)."""
    s = np.asarray(scores32, F32)
    n = s.shape[1]
    flat = s.reshape(-1)
    elig = np.flatnonzero(flat >= 0)
    order = elig[np.lexsort((elig, -flat[elig].astype(np.float64)))][:k]
    return order // n, order % n, flat[order]


def coarse_matching(ref_f, src_f, ref_mask, src_mask, k, dual=True):
    """The fp64 stage rounded to fp32, then its top-k: what rdm_coarse_matching_features computes.  Returns
    (row, col, score, fp64 score matrix)."""
    s64 = coarse_scores64(ref_f, src_f, ref_mask, src_mask, dual)
    return topk(s64.astype(F32), k) + (s64,)
