"""Generates tests/golden/feature_match.npz: the reference's descriptor protocol -- extract_corr_indices_from_feats (plain,
mutual, bilateral) and extract_correspondences_from_feats(..., return_feat_dist=True), geotransformer/utils/registration.py:222-277,
on get_nearest_neighbor's cKDTree (geotransformer/utils/pointcloud.py:11-22) -- imported with the shims of ref_import.py, CPU.
Build container only; the fixture travels, the reference not.

Inputs:
  (a) `crop9`, `small`: the FULL-resolution ref/src_feats_f and points_f of the reference forward on those two inputs (the
      forward_*.npz fixtures hold sub-sampled taps only, so the forward runs again here), of which ROWS evenly spaced rows per
      cloud are kept -- the whole tensors (about 2 x 2 500 x 256 floats per case) would not fit a committed file;
  (b) `random`: seeded normal features, 300 x 86 against 257 x 86 (no tile multiple anywhere), with random points.
For every case the generator asserts that no line's best and second-best float64 distances are exactly equal (cKDTree leaves
such ties open; this library takes the lowest index), and records the smallest gap it met.
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
sys.path.insert(0, os.path.join(REPO, 'tests'))
import feature_match_restatement as R  # noqa: E402

ROWS = 180


def main():
    cfg = ref_import.make_cfg()
    import gen_golden
    import geotransformer.utils.pointcloud as ref_pc
    from geotransformer.utils.registration import extract_corr_indices_from_feats, extract_correspondences_from_feats
    from model_infer import create_model
    from rdmnet_amd import config as my_config, weights
    from scipy.spatial import cKDTree

    class _Tree(cKDTree):  # the reference targets a scipy whose query() still takes n_jobs
        def query(self, x, k=1, n_jobs=None, **kw):
            return super().query(x, k=k, workers=-1 if n_jobs == -1 else 1, **kw)
    ref_pc.cKDTree = _Tree

    my_cfg = my_config.make_cfg()
    cfg.neighbor_limits = list(my_cfg.neighbor_limits)
    torch.manual_seed(0)
    np.random.seed(0)
    model = create_model(cfg)
    model.eval()
    state = weights.synthetic_state_dict(my_cfg, seed=0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    scans = np.load(os.path.join(HERE, 'scans.npz'))

    cases = {}
    for tag, radius in (('crop9', 9.0), ('small', 10.0)):
        rp, sp = gen_golden.crop(scans['s000000'], radius), gen_golden.crop(scans['s000004'], radius)
        torch.set_num_threads(8)
        _, out, _ = gen_golden.run_reference(cfg, model, rp, sp)
        full = {k: gen_golden.np_(out[k]) for k in ('ref_points_f', 'src_points_f', 'ref_feats_f', 'src_feats_f')}
        print(tag, 'full resolution:', full['ref_feats_f'].shape, full['src_feats_f'].shape)
        rows_r = np.linspace(0, len(full['ref_feats_f']) - 1, ROWS).round().astype(np.int64)
        rows_s = np.linspace(0, len(full['src_feats_f']) - 1, ROWS).round().astype(np.int64)
        cases[tag] = (full['ref_points_f'][rows_r], full['src_points_f'][rows_s], full['ref_feats_f'][rows_r],
                      full['src_feats_f'][rows_s])
    rng = np.random.default_rng(20240607)
    cases['random'] = (rng.standard_normal((300, 3)).astype(np.float32), rng.standard_normal((257, 3)).astype(np.float32),
                       rng.standard_normal((300, 86)).astype(np.float32), rng.standard_normal((257, 86)).astype(np.float32))

    fx = {'names': np.array(list(cases))}
    for tag, (rp, sp, rf, sf) in cases.items():
        assert rf.dtype == sf.dtype == np.float32 and rp.dtype == np.float32
        gaps = []
        for a, b in ((rf, sf), (sf, rf)):  # no exact float64 tie between a line's two best
            d = np.sort(R.sq_dists(a, b), axis=1)
            assert (d[:, 1] > d[:, 0]).all(), (tag, 'a best and a second-best distance are exactly equal')
            gaps.append(float((d[:, 1] - d[:, 0]).min()))
        fx[f'{tag}/min_gap'] = np.float64(min(gaps))
        fx[f'{tag}/ref_points'], fx[f'{tag}/src_points'], fx[f'{tag}/ref_feats'], fx[f'{tag}/src_feats'] = rp, sp, rf, sf
        for mode, kw in (('nearest', {}), ('mutual', {'mutual': True}), ('bilateral', {'bilateral': True})):
            ri, si = extract_corr_indices_from_feats(rf, sf, **kw)
            fx[f'{tag}/{mode}/ref_corr_indices'], fx[f'{tag}/{mode}/src_corr_indices'] = ri.astype(np.int64), si.astype(np.int64)
        for mode, mutual in (('nearest', False), ('mutual', True)):
            rc, sc, dist = extract_correspondences_from_feats(rp, sp, rf, sf, mutual=mutual, return_feat_dist=True)
            fx[f'{tag}/{mode}/ref_corr_points'], fx[f'{tag}/{mode}/src_corr_points'], fx[f'{tag}/{mode}/feat_dists'] = rc, sc, dist
            assert dist.dtype == np.float32
        print(tag, rf.shape, sf.shape, 'smallest best/second gap', fx[f'{tag}/min_gap'], '|a|^2 about',
              float((rf.astype(np.float64) ** 2).sum(1).mean()), 'mutual pairs', len(fx[f'{tag}/mutual/ref_corr_indices']))
    path = os.path.join(HERE, 'feature_match.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
