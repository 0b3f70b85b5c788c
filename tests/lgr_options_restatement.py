"""CPU restatement of LocalGlobalRegistration with every option of cfg.fine_matching (geotransformer/modules/geotransformer/
local_global_registration.py:49-91, :145-202, :229-243), as rdm_lgr_options defines what the reference leaves open:

  * among equal values at a k-th boundary the LOWEST index is kept (torch.topk does not say): lowest column for a row, lowest
    row for a column, lowest position in nonzero order for correspondence_limit;
  * the verification set of correspondence_limit stays in nonzero order (torch.topk returns it by descending score).

Arithmetic is the reference's (fp32 torch, fp32 torch.svd through oracle.forward.procrustes); oracle.forward.lgr is the
k = 1 / dustbin / non-mutual case of this file and stays the yardstick of that configuration.  `decisions` measures how far
every entry's membership is from flipping; `verification_set` and `final_inliers` serve the float64 pose bound of the tests.
"""
import itertools

import numpy as np
import torch

OPTION_KEYS = ('topk', 'mutual', 'use_dustbin', 'confidence_threshold', 'use_global_score', 'correspondence_limit')
UNDECIDED = 3e-7  # relative distance below which fp32 round-off of exp() may decide a comparison either way (~2.5 ulp)


def options(topk=1, mutual=False, use_dustbin=True, confidence_threshold=0.0, use_global_score=False, correspondence_limit=None):
    return dict(topk=topk, mutual=mutual, use_dustbin=use_dustbin, confidence_threshold=confidence_threshold,
                use_global_score=use_global_score, correspondence_limit=correspondence_limit)


def first_k(x, k, dim):
    """Bool mask of the k first entries along `dim` in the order (value descending, index ascending)."""
    idx = x.sort(dim=dim, descending=True, stable=True).indices.narrow(dim, 0, k)
    return torch.zeros_like(x, dtype=torch.bool).scatter_(dim, idx, True)


def score_matrix(log_scores, opt):
    """exp of what the forward hands LGR: the Sinkhorn output, or its K x K block without the dustbin (model_infer.py:319-320)."""
    return torch.exp(log_scores if opt['use_dustbin'] else log_scores[:, :-1, :-1])


def correspondence_matrix(score, ref_mask, src_mask, opt):
    """:49-91.  score: (B, K+1, K+1) with the dustbin, (B, K, K) without.  -> bool (B, K, K)."""
    k = opt['topk']
    if opt['use_dustbin']:
        bar_r, bar_c = score[:, :, -1:], score[:, -1:, :]
    else:
        bar_r = bar_c = torch.tensor(opt['confidence_threshold'], dtype=score.dtype)
    ref_side = first_k(score, k, 2) & (score > bar_r)
    src_side = first_k(score, k, 1) & (score > bar_c)
    corr = (ref_side & src_side) if opt['mutual'] else (ref_side | src_side)
    if opt['use_dustbin']:
        corr = corr[:, :-1, :-1]
    return corr & (ref_mask[:, :, None] & src_mask[:, None, :])


def verification_set(scores, limit, by_score=False):
    """Positions of the correspondences the hypotheses are scored and the pose is refined on (:152-160), ascending -- or, with
    `by_score`, in the reference's order (descending score): the same set, fp32 sums in the reference's order."""
    scores = torch.as_tensor(scores)
    n = scores.shape[0]
    if limit is None or n <= limit:
        return torch.arange(n)
    first = scores.sort(descending=True, stable=True).indices[:limit]
    return first if by_score else first.sort().values


def lgr(ref_knn, src_knn, ref_mask, src_mask, log_scores, global_scores, fm, opt, force_best=None, by_score=False):
    """-> dict: indices (C, 3) int64 (patch, i, j) in nonzero order, ref_corr_points, src_corr_points, corr_scores (all C),
    transform (4, 4), verification (positions), chunks, and -- when a patch reaches correspondence_threshold -- hypotheses,
    inlier_counts, best.  `fm`: acceptance_radius, correspondence_threshold, num_refinement_steps.  `force_best` (test
    probe, as oracle.forward.lgr): refine from that hypothesis instead of the first argmax of the inlier counts.  `by_score`:
    the verification set in the reference's order (see verification_set)."""
    from oracle import forward as ofw
    score = score_matrix(log_scores, opt)
    corr = correspondence_matrix(score, ref_mask, src_mask, opt)
    if opt['use_dustbin']:
        score = score[:, :-1, :-1]
    if opt['use_global_score']:
        score = score * global_scores.view(-1, 1, 1)
    score = score * corr.float()
    bi, ri, si = torch.nonzero(corr, as_tuple=True)
    g_ref, g_src, g_sc = ref_knn[bi, ri], src_knn[bi, si], score[bi, ri, si]
    ver = verification_set(g_sc, opt['correspondence_limit'], by_score)
    ref_c, src_c, sc = g_ref[ver], g_src[ver], g_sc[ver]
    cuts = [0] + (torch.nonzero(bi[1:] != bi[:-1], as_tuple=True)[0] + 1).tolist() + [bi.shape[0]] if bi.shape[0] else [0]
    chunks = [(x, y) for x, y in zip(cuts[:-1], cuts[1:]) if y - x >= fm.correspondence_threshold]
    out = dict(indices=torch.stack([bi, ri, si], 1), ref_corr_points=g_ref, src_corr_points=g_src, corr_scores=g_sc,
               verification=ver, chunks=chunks)
    radius = fm.acceptance_radius
    if chunks:
        width = max(y - x for x, y in chunks)
        bs, br, bw = torch.zeros(len(chunks), width, 3), torch.zeros(len(chunks), width, 3), torch.zeros(len(chunks), width)
        for c, (x, y) in enumerate(chunks):  # fitted on ALL correspondences of the patch, scored on the verification set
            bs[c, :y - x], br[c, :y - x], bw[c, :y - x] = g_src[x:y], g_ref[x:y], g_sc[x:y]
        Ts = ofw.procrustes(bs, br, bw)
        inl = torch.linalg.norm(ref_c[None] - ofw._apply(Ts, src_c[None]), dim=2) < radius
        best = inl.sum(1).argmax() if force_best is None else torch.tensor(int(force_best))
        cur = sc * inl[best].float()
        out.update(hypotheses=Ts, inlier_counts=inl.sum(1), best=int(best))
    else:
        T0 = ofw.procrustes(src_c[None], ref_c[None], sc[None])[0]
        cur = sc * (torch.linalg.norm(ref_c - ofw._apply(T0, src_c), dim=1) < radius).float()
    T = ofw.procrustes(src_c[None], ref_c[None], cur[None])[0]
    for _ in range(fm.num_refinement_steps - 1):
        cur = sc * (torch.linalg.norm(ref_c - ofw._apply(T, src_c), dim=1) < radius).float()
        T = ofw.procrustes(src_c[None], ref_c[None], cur[None])[0]
    out['transform'] = T
    return out


def alternatives(ref_knn, src_knn, ref_mask, src_mask, log_scores, global_scores, fm, opt, within=1):
    """As tie_aware.lgr_alternatives: the un-forced run and [(hypothesis, pose)] for every hypothesis whose inlier count is
    within `within` of the best."""
    args = (ref_knn, src_knn, ref_mask, src_mask, log_scores, global_scores, fm, opt)
    run = lgr(*args)
    if 'inlier_counts' not in run:
        return run, [(-1, run['transform'].numpy())]
    counts = run['inlier_counts'].numpy()
    near = [int(i) for i in np.nonzero(counts >= counts.max() - within)[0]]
    return run, [(i, lgr(*args, force_best=i)['transform'].numpy()) for i in near]


def _rank_margin(score, k, dim):
    """Per entry: relative distance to the value it would have to cross to enter / leave the k first of its line."""
    n = score.shape[dim]
    if k >= n:
        return torch.full_like(score, float('inf'))
    srt = score.sort(dim=dim, descending=True, stable=True).values
    vk, vk1 = srt.narrow(dim, k - 1, 1), srt.narrow(dim, k, 1)
    inside = first_k(score, k, dim)
    other = torch.where(inside, vk1.expand_as(score), vk.expand_as(score))
    return (score - other).abs() / torch.maximum(score, other).clamp_min(1e-38)


def decisions(log_scores, ref_mask, src_mask, opt):
    """-> (corr, undecided), bool (B, K, K).  An entry is undecided when flipping some of the comparisons that lie within
    UNDECIDED (relative) -- rank against the line's k-th / (k+1)-th value, value against the dustbin entry or the threshold,
    on either side -- changes whether it is a correspondence.  Entries equal to 0 and masked lines are decided (not)."""
    score = score_matrix(log_scores, opt).double()
    k = opt['topk']
    if opt['use_dustbin']:
        bar_r, bar_c = score[:, :, -1:].expand_as(score), score[:, -1:, :].expand_as(score)
    else:
        bar_r = bar_c = torch.full_like(score, float(np.float32(opt['confidence_threshold'])))
    vals = [first_k(score, k, 2), score > bar_r, first_k(score, k, 1), score > bar_c]
    rel = lambda a, b: (a - b).abs() / torch.maximum(a, b).clamp_min(1e-38)
    near = [_rank_margin(score, k, 2) < UNDECIDED, rel(score, bar_r) < UNDECIDED,
            _rank_margin(score, k, 1) < UNDECIDED, rel(score, bar_c) < UNDECIDED]
    can_true, can_false = torch.zeros_like(vals[0]), torch.zeros_like(vals[0])
    for a in itertools.product((False, True), repeat=4):
        ok = torch.ones_like(vals[0])
        for x, v, n in zip(a, vals, near):
            ok &= n | (v == x)
        f = (a[0] and a[1] and a[2] and a[3]) if opt['mutual'] else ((a[0] and a[1]) or (a[2] and a[3]))
        if f:
            can_true |= ok
        else:
            can_false |= ok
    live = (ref_mask[:, :, None] & src_mask[:, None, :])
    if opt['use_dustbin']:
        can_true, can_false, score = can_true[:, :-1, :-1], can_false[:, :-1, :-1], score[:, :-1, :-1]
    live = live & (score > 0)
    corr = correspondence_matrix(score_matrix(log_scores, opt), ref_mask, src_mask, opt)
    return corr, can_true & can_false & live


def limit_gap(scores, limit):
    """Relative gap between the L-th and (L+1)-th largest score (inf when the limit does not bite)."""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    if limit is None or len(s) <= limit:
        return float('inf')
    return float((s[limit - 1] - s[limit]) / max(s[limit - 1], 1e-38))


def final_inliers(T, ref_c, src_c, radius):
    """Residuals of the verification set under pose T in float64 -> (inlier mask, smallest |residual - radius|)."""
    T, ref_c, src_c = (np.asarray(x, np.float64) for x in (T, ref_c, src_c))
    res = np.linalg.norm(ref_c - (src_c @ T[:3, :3].T + T[:3, 3]), axis=1)
    return res < radius, float(np.abs(res - radius).min()) if len(res) else float('inf')


def tie_patch():
    """LGR inputs of one 6 x 6 patch (+ dustbin) with exact ties at every boundary the tie rule decides: equal log scores give
    equal S = exp(log score) whatever the exp."""
    a, b, c, z = np.log(0.30), np.log(0.20), np.log(0.10), np.log(0.01)
    L = np.full((1, 7, 7), z, np.float32)
    L[0, 0, [1, 3, 4]] = a          # row 0: three equal maxima -> k = 2 keeps columns 1, 3
    L[0, 1, [0, 2]] = b             # row 1: two equal maxima
    L[0, [2, 4, 5], 5] = a          # column 5: three equal maxima -> k = 2 keeps rows 2, 4
    L[0, 3, 2] = c
    L[0, :6, 6] = np.log(0.05)      # dustbin column
    L[0, 6, :6] = np.log(0.05)      # dustbin row
    pts = np.arange(36, dtype=np.float32).reshape(1, 6, 3 * 2)[:, :, :3] + np.float32(0.25)
    return (torch.from_numpy(pts.copy()), torch.from_numpy(pts[:, ::-1].copy() * np.float32(1.5)), torch.ones(1, 6, dtype=torch.bool),
            torch.ones(1, 6, dtype=torch.bool), torch.from_numpy(L), torch.tensor([0.5]))


# ---------------------------------------------------------------------------- the fixture (tests/golden/lgr_options.npz)
def fixture_entries(golden_dir):
    """[(case, set name)] of tests/golden/lgr_options.npz."""
    import os
    z = np.load(os.path.join(golden_dir, 'lgr_options.npz'))
    return sorted({tuple(k.split('/')[:2]) for k in z.files})


def fixture_entry(golden_dir, case, name):
    """-> (options dict, {field: array}) of one fixture entry."""
    import os
    z = np.load(os.path.join(golden_dir, 'lgr_options.npz'))
    p = f'{case}/{name}/'
    f = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    o = f['options']
    return options(int(o[0]), bool(o[1]), bool(o[2]), float(o[3]), bool(o[4]), None if o[5] < 0 else int(o[5])), f


def golden_inputs(golden_dir, case):
    """The LGR inputs a forward golden holds: (ref knn points, src knn points, ref masks, src masks, matching scores
    (B, K+1, K+1), superpoint-pair scores) as CPU tensors."""
    import os
    from sampling import expand_scores
    g = np.load(os.path.join(golden_dir, f'forward_{case}.npz'))
    rm, sm = g['out/ref_node_corr_knn_masks'], g['out/src_node_corr_knn_masks']
    ms = torch.from_numpy(expand_scores(g['out/matching_scores'], rm, sm))
    return (torch.from_numpy(g['out/ref_node_corr_knn_points']), torch.from_numpy(g['out/src_node_corr_knn_points']),
            torch.from_numpy(rm).bool(), torch.from_numpy(sm).bool(), ms, torch.from_numpy(g['tap/node_corr_scores']))


def compare_correspondences(got_idx, f, cap=0.02):
    """The fixture's rule: exact entries -- the same triples in the same order; tie-aware entries -- every decided entry
    decided as the reference did, and at most `cap` of C undecided.  -> number of triples that differ."""
    want = {tuple(r) for r in f['indices'].astype(np.int64).tolist()}
    got_list = [tuple(r) for r in np.asarray(got_idx, np.int64).tolist()]
    got = set(got_list)
    assert len(got) == len(got_list)
    if bool(f['exact']):
        assert got_list == [tuple(r) for r in f['indices'].astype(np.int64).tolist()], len(got ^ want)
        return 0
    und = {tuple(r) for r in f['undecided'].astype(np.int64).tolist()}
    assert len(und) <= cap * len(want), (len(und), len(want))
    assert (got ^ want) <= und, sorted((got ^ want) - und)[:8]
    return len(got ^ want)
