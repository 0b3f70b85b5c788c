"""Float64 brute-force restatement of the descriptor protocol (geotransformer/utils/registration.py:222-277 on
get_nearest_neighbor, geotransformer/utils/pointcloud.py:11-22), numpy only: the definition rdm_feature_match is held to.

The nearest row is the argmin over j of sum_c (a_ic - b_jc)^2 evaluated in float64 on the float32 inputs; among exactly equal
distances the lowest index wins (np.argmin's rule; cKDTree leaves ties open).  The distance of a pair is sqrt of that float64 sum
rounded to float32.
"""
import numpy as np


def sq_dists(a, b, block=256):
    """[N, M] float64 squared distances in the direct difference form."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(0, a.shape[0], block):
        d = a[i:i + block, None, :] - b[None, :, :]
        out[i:i + block] = np.einsum('nmc,nmc->nm', d, d)
    return out


def nearest(a, b):
    """-> (index int64 [N], distance float32 [N]) of the nearest row of b for every row of a."""
    if a.shape[0] == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.float32)
    d = sq_dists(a, b)
    idx = d.argmin(axis=1).astype(np.int64)  # (first minimum = lowest index)
    return idx, np.sqrt(d[np.arange(len(idx)), idx]).astype(np.float32)


def corr_indices(ref_feats, src_feats, mutual=False, bilateral=False, return_dist=False):
    """extract_corr_indices_from_feats: same semantics and output order; with return_dist also the pairs' distances."""
    nn_ref, d_ref = nearest(ref_feats, src_feats)
    n, m = ref_feats.shape[0], src_feats.shape[0]
    if mutual or bilateral:
        nn_src, d_src = nearest(src_feats, ref_feats)
    if mutual:
        keep = nn_src[nn_ref] == np.arange(n)
        ri, si, dist = np.arange(n, dtype=np.int64)[keep], nn_ref[keep], d_ref[keep]
    elif bilateral:
        ri = np.concatenate([np.arange(n, dtype=np.int64), nn_src])
        si = np.concatenate([nn_ref, np.arange(m, dtype=np.int64)])
        dist = np.concatenate([d_ref, d_src])
    else:
        ri, si, dist = np.arange(n, dtype=np.int64), nn_ref, d_ref
    return (ri, si, dist) if return_dist else (ri, si)


def correspondences(ref_points, src_points, ref_feats, src_feats, mutual=False, bilateral=False, return_feat_dist=False):
    """extract_correspondences_from_feats (plus `bilateral`)."""
    ri, si, dist = corr_indices(ref_feats, src_feats, mutual, bilateral, return_dist=True)
    out = [ref_points[ri], src_points[si]]
    if return_feat_dist:
        out.append(dist)
    return out


def ulp_diff(x, y):
    """Distance in float32 units in the last place between two non-negative float32 arrays."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


def nearest_fast(a, b):
    """nearest() for shapes whose [N, M, C] difference tensor is too slow to form: the float64 expansion |a|^2 + |b|^2 - 2 a.b
    (error <= (C + 5) 2^-53 (|a|^2 + |b|^2), the fp32 bound of feature_match.hip with u = 2^-53: below 3e-13 relative for
    C <= 1024) selects, per line, every candidate within 1e-9 (|a_i|^2 + max |b|^2) of its minimum -- thousands of times that
    error --, and the direct difference form decides among them.  Same answer as nearest(), candidates in ascending index."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = (a64 * a64).sum(1), (b64 * b64).sum(1)
    e = na[:, None] + nb[None, :] - 2.0 * (a64 @ b64.T)
    tol = 1e-9 * (na + nb.max())
    idx = np.empty((a64.shape[0],), np.int64)
    d2 = np.empty((a64.shape[0],), np.float64)
    for i in range(a64.shape[0]):
        cand = np.nonzero(e[i] <= e[i].min() + tol[i])[0]
        diff = a64[i][None, :] - b64[cand]
        d = np.einsum('mc,mc->m', diff, diff)
        k = int(d.argmin())
        idx[i], d2[i] = cand[k], d[k]
    return idx, np.sqrt(d2).astype(np.float32)
