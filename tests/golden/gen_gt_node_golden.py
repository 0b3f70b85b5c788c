"""Generates tests/golden/gt_node_corr.npz by running the REFERENCE's evaluation forward (experiments/model.py, the model
test.py runs) on CPU with the seeded synthetic weights, through the import shims of ref_import.py.  Build container only;
the fixture travels, the reference not.

Per case `<tag>/...` it stores what get_node_correspondences (geotransformer/modules/registration/matching.py:252-350)
received at experiments/model.py:283-295 and what it returned:
  * inputs: nodes [M,3] / [N,3], the patch point indices [M,128] (int16) into each cloud's fine points (pad index = n, a
    zero row, exactly the reference's index_select on the padded points), node masks, patch masks, the ground-truth
    transform and the radius.  The fine points themselves (level 1 of the collate, ~750 KB) are not stored: a test
    rebuilds them from the case's input clouds (`case_clouds`, committed fixtures) with this repository's collate and
    checks them against the stored sha256 of the reference's `points_f` halves (`ref_points_f_sha256`, `n_ref_points_f`);
  * outputs: corr_indices int64 [C,2], corr_overlaps f32 [C];
  * `B`, the number of candidate patch pairs that pass the enclosing-sphere test, their (ref, src) indices, and per
    candidate the smallest margin |d^2 - r^2| over its valid point pairs (the reference's own fp32 d^2), so that a test
    can tell a disagreement from a tie.
`e2e/...` holds the output_dict keys gt_node_corr_* of the synth0 forward and the nodes they were computed on.

    python tests/golden/gen_gt_node_golden.py            # all cases (a few minutes of CPU)
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import ref_import  # noqa: E402


def np_(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def known_transform():
    """The transform of the bundled-scan case: src = T^-1 ref, so T maps src -> ref as the dataset's `transform` does."""
    yaw = np.deg2rad(10.0)
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [3.0, -1.0, 0.2]
    return T


def case_clouds(golden_dir):
    """tag -> (ref cloud, src cloud, transform src -> ref), all from committed fixtures: the forward_*.npz inputs of
    gen_golden.py and the bundled scan 0 moved by known_transform().  tests/test_gt_node_corr_gpu.py uses the same."""
    cases = {}
    for tag, t_key in (('synth0', 'T0'), ('synth3', 'T3'), ('lowoverlap', None), ('dense20k', None)):
        f = np.load(os.path.join(golden_dir, f'forward_{tag}.npz'))
        cases[tag] = [f['ref_points_in'], f['src_points_in'], None]
    synth = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    cases['synth0'][2], cases['synth3'][2] = synth['T0'], synth['T3']
    T_known = known_transform()
    s0 = np.load(os.path.join(golden_dir, 'scans.npz'))['s000000']
    s0_moved = ((s0.astype(np.float64) - T_known[:3, 3]) @ T_known[:3, :3]).astype(np.float32)  # T^-1 applied
    cases['scan0_known'] = [s0, s0_moved, T_known]
    return cases


def main():
    cfg = ref_import.make_cfg()
    import model as ref_model
    from geotransformer.modules.ops import pairwise_distance, apply_transform
    from geotransformer.utils.data import registration_collate_fn_stack_mode
    from rdmnet_amd import config as my_config, synthetic, weights

    my_cfg = my_config.make_cfg()
    cfg.neighbor_limits = list(my_cfg.neighbor_limits)
    torch.manual_seed(0)
    np.random.seed(0)
    net = ref_model.create_model(cfg)
    net.eval()
    state = weights.synthetic_state_dict(my_cfg, seed=0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)

    captured = []
    orig = ref_model.get_node_correspondences

    def spy(*args, **kwargs):
        out = orig(*args, **kwargs)
        captured.append((args, kwargs, out))
        return out

    ref_model.get_node_correspondences = spy

    cases = case_clouds(HERE)
    # (the low-overlap and dense clouds are the ones rdmnet_amd.synthetic makes; their transforms come from it too)
    cases['lowoverlap'][2] = synthetic.make_low_overlap_pair(0)[2]
    cases['dense20k'][2] = synthetic.make_pair(40, target_points=20000)[2]
    torch.set_num_threads(8)
    fx = {}
    for tag, (rp, sp, T) in cases.items():
        item = {'seq_id': 0, 'ref_frame': 0, 'src_frame': 1, 'ref_points': rp, 'src_points': sp,
                'ref_feats': np.ones((rp.shape[0], 1), np.float32), 'src_feats': np.ones((sp.shape[0], 1), np.float32),
                'transform': np.asarray(T, np.float32)}
        data = registration_collate_fn_stack_mode([item], cfg.backbone.num_stages, cfg.backbone.init_voxel_size,
                                                  cfg.backbone.init_radius, cfg.neighbor_limits)
        for key in ('neighbors', 'subsampling', 'upsampling'):
            data[key] = [x.contiguous() for x in data[key]]
        data['testing'] = True
        captured.clear()
        with torch.no_grad():
            out = net(data)
        assert len(captured) == 1, tag
        args, kwargs, (corr, ovl) = captured[0]
        ref_nodes, src_nodes, ref_knn_pts, src_knn_pts, transform, radius = args
        assert torch.equal(corr, out['gt_node_corr_indices']) and torch.equal(ovl, out['gt_node_corr_overlaps'])
        n_f = int(data['lengths'][1][0])
        pts_f = data['points'][1]
        ref_f, src_f = pts_f[:n_f], pts_f[n_f:]
        k = my_cfg.model.num_points_in_patch
        # the patch indices behind the gathered knn points (model.py:268-273): recomputed with the reference's own grouping
        from geotransformer.modules.ops import point_to_node_partition, index_select
        _, r_nm, r_idx, r_km = point_to_node_partition(ref_f, ref_nodes, k)
        _, s_nm, s_idx, s_km = point_to_node_partition(src_f, src_nodes, k)
        for f, idx, knn in ((ref_f, r_idx, ref_knn_pts), (src_f, s_idx, src_knn_pts)):
            assert torch.equal(index_select(torch.cat([f, torch.zeros_like(f[:1])]), idx, dim=0), knn), tag
        assert torch.equal(r_nm, kwargs['ref_masks']) and torch.equal(s_km, kwargs['src_knn_masks']), tag

        # candidates and margins, with the reference's own arithmetic
        inter = orig(*args, **kwargs, return_mask=True)
        sel_r, sel_s = torch.nonzero(inter, as_tuple=True)
        B = sel_r.shape[0]
        src_knn_t = apply_transform(src_knn_pts, transform)
        r2 = np.float32(radius ** 2)
        margins = np.empty(B, np.float64)
        for a in range(0, B, 512):
            rs, ss = sel_r[a:a + 512], sel_s[a:a + 512]
            d = pairwise_distance(ref_knn_pts[rs], src_knn_t[ss]).double()
            valid = kwargs['ref_knn_masks'][rs].unsqueeze(2) & kwargs['src_knn_masks'][ss].unsqueeze(1)
            gap = (d - float(r2)).abs().masked_fill(~valid, np.inf)
            margins[a:a + 512] = gap.flatten(1).min(1)[0].numpy()
        p = tag + '/'
        assert max(ref_f.shape[0], src_f.shape[0]) < 2 ** 15  # (int16 indices)
        fx.update({p + 'ref_nodes': np_(ref_nodes), p + 'src_nodes': np_(src_nodes),
                   p + 'ref_points_f_sha256': np.array(hashlib.sha256(np_(ref_f).tobytes()).hexdigest()),
                   p + 'src_points_f_sha256': np.array(hashlib.sha256(np_(src_f).tobytes()).hexdigest()),
                   p + 'n_ref_points_f': np.int64(ref_f.shape[0]), p + 'n_src_points_f': np.int64(src_f.shape[0]),
                   p + 'ref_knn_indices': np_(r_idx).astype(np.int16), p + 'src_knn_indices': np_(s_idx).astype(np.int16),
                   p + 'ref_masks': np_(kwargs['ref_masks']), p + 'src_masks': np_(kwargs['src_masks']),
                   p + 'ref_knn_masks': np_(kwargs['ref_knn_masks']), p + 'src_knn_masks': np_(kwargs['src_knn_masks']),
                   p + 'transform': np_(transform), p + 'pos_radius': np.float64(radius),
                   p + 'corr_indices': np_(corr), p + 'corr_overlaps': np_(ovl),
                   p + 'B': np.int64(B), p + 'cand_indices': np.stack([np_(sel_r), np_(sel_s)], 1).astype(np.int16),
                   p + 'cand_margin': margins.astype(np.float32)})
        if tag == 'synth0':
            fx.update({'e2e/ref_points_c': np_(out['ref_points_c']), 'e2e/src_points_c': np_(out['src_points_c']),
                       'e2e/gt_node_corr_indices': np_(out['gt_node_corr_indices']),
                       'e2e/gt_node_corr_overlaps': np_(out['gt_node_corr_overlaps']),
                       'e2e/transform': np.asarray(T, np.float32)})  # (the clouds: synthetic_pairs.npz ref0 / src0)
        tight = int((margins <= 2 * np.spacing(r2)).sum())
        print(f'{tag}: M={ref_nodes.shape[0]} N={src_nodes.shape[0]} B={B} C={corr.shape[0]} '
              f'candidates within 2 ulp of r^2: {tight}', flush=True)
    np.savez_compressed(os.path.join(HERE, 'gt_node_corr.npz'), **fx)


if __name__ == '__main__':
    main()
