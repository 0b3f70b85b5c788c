"""Generates tests/golden/forward_topk_synth0.npz: the REFERENCE's RDMNet.forward with top-k attention in the second
3DRoFormer (cfg.thdroformer.k2, rdmnet/thdroformer/thdroformer.py:20-40), imported from the reference with the shims of
ref_import.py and run on CPU.  Build container only; the fixture travels, the reference not.

The case is the 15 m crop of synth0 with weight seed 0.  k2 is chosen here, layer by layer, so that the selection of every
row is clear of fp32 round-off: the scores of a row are off by ~1e-6 of their largest in any fp32 evaluation, and at full
size (213 + 226 superpoints, 4 heads) the smallest relative gap between the k-th and (k+1)-th score over a layer's rows is
~3e-7 whatever the fraction -- a selection any summation order can flip.  On the crop, for each self layer in turn (the
earlier ones fixed), the fraction with the largest smallest gap is taken from a grid:
  - layers 0 and 1: interior fractions 0.20 .. 0.44 and 0.45 .. 0.75;
  - layer 2: the fractions f near m / n (m / n, m / n to 2 or 3 decimals, or the double just below m / n) whose product
    with a cloud's count n falls just below the integer m in double, so the reference keeps int(n * f) = m - 1 keys of that
    cloud, not m;
  - layer 3: 1.0 (every key kept: the dense softmax through the top-k path).
The file holds the taps and outputs of gen_golden.py (same names, same row sampling; not the matching scores) and, from
the module-level dynamic_attention wrapped in-process, for two self layers (self layers 0 and 2 of the ref cloud): the
post-RoPE q, k, v the reference attended with, its output, the selected set (torch.topk rerun on the captured scores:
the non-zeros of the reference's probabilities would miss kept keys whose probability underflows to 0), and the kept
count.  `attn/min_rel_gap` is the smallest (s_k - s_k+1) / max|s| over every row and head of every top-k call of the run (all layers, both clouds).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import ref_import  # noqa: E402
import gen_golden  # noqa: E402
sys.path.insert(0, os.path.join(REPO, 'tests'))
from sampling import sample  # noqa: E402

CROP = 15.0
GRID = [np.round(np.arange(0.20, 0.445, 0.01), 2).tolist(), np.round(np.arange(0.45, 0.755, 0.01), 2).tolist()]
CAPTURE = {0: 'l0_ref', 4: 'l2_ref'}  # index of the top-k call (layer-major, ref then src) -> fixture prefix
np_ = gen_golden.np_


def min_gap(calls, which):
    """Smallest (s_k - s_k+1) / max|s| over the rows and heads of the top-k calls `which` (interior kept counts only)."""
    gaps = [np.inf]
    for c in which:
        q, k, _, _, f = calls[c]
        n = q.shape[2]
        kc = int(n * f)
        if 0 < kc < n:
            scores = torch.einsum('bhnd,bhmd->bhnm', q, k) / q.shape[3] ** .5
            srt = scores.sort(dim=3, descending=True).values
            gaps.append(float(((srt[..., kc - 1] - srt[..., kc]) / scores.abs().amax(dim=3).clamp_min(1e-30)).min()))
    return min(gaps)


def main():
    cfg = ref_import.make_cfg()
    K2 = [1.0, 1.0, 1.0, 1.0]  # the list every self layer of transformer #2 holds (edited in place by the search)
    cfg.thdroformer.k2 = K2
    from model_infer import create_model
    from rdmnet.thdroformer import thdroformer as thd
    from rdmnet_amd import config as my_config, weights
    from oracle import forward as ofw

    my_cfg = my_config.make_cfg()
    cfg.neighbor_limits = list(my_cfg.neighbor_limits)
    torch.manual_seed(0)
    np.random.seed(0)
    model = create_model(cfg)
    model.eval()
    state = weights.synthetic_state_dict(my_cfg, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    holders = [m for m in model.transformer2.modules() if getattr(m, 'k', None) is not None]
    assert holders and all(m.k is K2 for m in holders)

    calls = []
    orig = thd.dynamic_attention

    def wrapped(query, key, value, k):
        out, probs = orig(query, key, value, k)
        if k is not None:
            calls.append((query.clone(), key.clone(), value.clone(), out.clone(), k))
        return out, probs

    synth = np.load(os.path.join(HERE, 'synthetic_pairs.npz'))
    rp, sp = gen_golden.crop(synth['ref0'], CROP), gen_golden.crop(synth['src0'], CROP)
    t2_in = {}
    pre = model.transformer2.register_forward_pre_hook(lambda _m, a, kw: t2_in.update(args=a, kwargs=kw), with_kwargs=True)
    thd.dynamic_attention = wrapped
    try:
        torch.set_num_threads(8)
        gen_golden.run_reference(cfg, model, rp, sp)  # transformer #2's inputs do not depend on k2
        pre.remove()
        counts = (calls[0][0].shape[2], calls[1][0].shape[2])
        GRID.append(sorted({f for n in counts for m in range(1, n)
                            for f in (m / n, round(m / n, 2), round(m / n, 3), float(np.nextafter(m / n, 0)))
                            if abs(n * f - m) < 1e-9 and int(n * f) < m and 0.1 < f < 0.9}))
        assert GRID[2], counts
        for layer, grid in enumerate(GRID):
            best = (-1.0, None)
            for f in grid:
                K2[layer] = f
                calls.clear()
                with torch.no_grad():
                    model.transformer2(*t2_in['args'], **t2_in['kwargs'])
                best = max(best, (min_gap(calls, (2 * layer, 2 * layer + 1)), f))
            K2[layer] = best[1]
            print(f'self layer {layer}: k2 = {best[1]!r}, smallest relative gap {best[0]:.3e}')
        calls.clear()
        data, out, taps = gen_golden.run_reference(cfg, model, rp, sp)
        captured, calls[:] = list(calls), []
        torch.set_num_threads(1)
        _, out1, taps1 = gen_golden.run_reference(cfg, model, rp, sp)
        torch.set_num_threads(8)
    finally:
        thd.dynamic_attention = orig
    assert len(captured) == 2 * len(K2), len(captured)

    fx = {'ref_points_in': rp, 'src_points_in': sp, 'weight_seed': np.int64(0), 'k2': np.asarray(K2, np.float64)}
    for i in range(5):
        fx[f'lengths{i}'] = np_(data['lengths'][i])
    for n, v in taps.items():
        if n.startswith('encoder.'):
            fx[f'tap/{n}'] = sample(np_(v))
    fx['tap/t1_ref'], fx['tap/t1_src'] = sample(np_(taps['transformer'][0][0])), sample(np_(taps['transformer'][1][0]))
    fx['tap/t2_ref'], fx['tap/t2_src'] = sample(np_(taps['transformer2'][0][0])), sample(np_(taps['transformer2'][1][0]))
    fx['tap/vote_xyz'], fx['tap/vote_feats'] = np_(taps['vote'][0]), sample(np_(taps['vote'][1]))
    fx['tap/nms_mask'] = np_(taps['nms'])
    fx['tap/decoder'] = sample(np_(taps['decoder'][0]))
    fx['tap/node_corr_scores'] = np_(taps['coarse_matching'][2])
    for k, v in out.items():
        a = np_(v)
        if k in ('ref_points', 'src_points', 'ref_points_f', 'src_points_f'):
            continue
        if k in ('ref_feats_f', 'src_feats_f', 'ref_p2p_scores_c', 'src_p2p_scores_c', 'ref_feats_c', 'src_feats_c'):
            a = sample(a)
        if k == 'matching_scores':  # (1.5 MB even compacted; the tests judge what is computed from it: correspondences, pose)
            continue
        fx['out/' + k] = a

    # ---- the top-k calls: kept counts, the selection margin, and two layers' operands / outputs / selected sets
    kcs = []
    for c, (q, k, v, o, f) in enumerate(captured):
        n = q.shape[2]
        kc = int(n * f)  # thdroformer.py:27
        kcs.append(kc)
        scores = torch.einsum('bhnd,bhmd->bhnm', q, k) / q.shape[3] ** .5  # thdroformer.py:23
        if c in CAPTURE:
            tag = CAPTURE[c]
            sel = np.zeros(scores.shape[1:], bool)
            if kc > 0:
                idx = scores.topk(kc, dim=3, largest=True, sorted=False).indices[0]
                np.put_along_axis(sel, np_(idx), True, axis=2)
            fx[f'attn/{tag}/q'], fx[f'attn/{tag}/k'], fx[f'attn/{tag}/v'] = np_(q[0]), np_(k[0]), np_(v[0])
            fx[f'attn/{tag}/out'] = np_(o[0])
            fx[f'attn/{tag}/selected'] = sel
            fx[f'attn/{tag}/keep'] = np.int64(kc)
    fx['attn/keep_counts'] = np.asarray(kcs, np.int64)  # per call: layer-major, ref then src
    fx['attn/min_rel_gap'] = np.float64(min_gap(captured, range(len(captured))))
    fx['attn/n'] = np.asarray([captured[0][0].shape[2], captured[1][0].shape[2]], np.int64)  # superpoints: ref, src

    # ---- pose margin of the reference's own registration and the poses of near-tied hypotheses (as gen_golden.py)
    lgr_in = (out['ref_node_corr_knn_points'], out['src_node_corr_knn_points'], out['ref_node_corr_knn_masks'],
              out['src_node_corr_knn_masks'], out['matching_scores'], my_cfg)
    rc, sc2, cs, T, linfo = ofw.lgr(*lgr_in)
    counts = linfo['inlier_counts'].numpy()
    near = [int(i) for i in np.nonzero(counts >= counts.max() - 1)[0]]
    fx['lgr/inlier_counts'] = counts.astype(np.int64)
    fx['lgr/best'] = np.int64(linfo['best'])
    fx['lgr/alt_hypotheses'] = np.asarray(near, np.int64)
    fx['lgr/alt_transforms'] = np.stack([np_(ofw.lgr(*lgr_in, force_best=i)[3]) for i in near])
    # ---- the reference against itself at 1 thread
    pairs8 = set(zip(np_(out['ref_node_corr_indices']).tolist(), np_(out['src_node_corr_indices']).tolist()))
    pairs1 = set(zip(np_(out1['ref_node_corr_indices']).tolist(), np_(out1['src_node_corr_indices']).tolist()))
    fx['self/node_corr_symmetric_difference'] = np.int64(len(pairs8 ^ pairs1))
    fx['self/nms_mask_equal'] = np.bool_(np.array_equal(np_(taps['nms']), np_(taps1['nms'])))
    fx['self/transform_1_thread'] = np_(out1['estimated_transform'])
    fx['self/n_corr_1_thread'] = np.int64(out1['corr_scores'].shape[0])
    fx['self/corr_symmetric_difference'] = np.int64(gen_golden.corr_symmetric_difference(out1, out))
    path = os.path.join(HERE, 'forward_topk_synth0.npz')
    np.savez_compressed(path, **fx)
    rre, rte = ofw.rre_rte(np_(out1['estimated_transform']), np_(out['estimated_transform']))
    print(f'{path}: k2 {K2}, keep counts {kcs}, min relative gap {float(fx["attn/min_rel_gap"]):.3e}, lgr margin '
          f'{int(np.sort(counts)[::-1][:2] @ [1, -1])}, self 8 vs 1 thread: node pairs {len(pairs8 ^ pairs1)}, corr '
          f'{int(fx["self/corr_symmetric_difference"])}, rre {rre:.2e} rte {rte:.2e}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
