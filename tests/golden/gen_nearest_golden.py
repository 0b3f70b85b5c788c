"""Generates tests/golden/nearest.npz: the reference's get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22, scipy's
cKDTree), compute_overlap, compute_modified_chamfer_distance and compute_registration_rmse
(geotransformer/utils/registration.py:136-197) imported with the shims of ref_import.py, CPU.
Build container only; the fixture travels, the reference not.

Cases (points go to the reference as float64 copies of the fp32 values, so its arithmetic is float64):
  (a) pairs 0 and 3 of tests/golden/synthetic_pairs.npz (ref*, src*, T*) under the ground-truth transform (`gt`) and under a pose
      0.5 degrees / 0.2 m off it (`off`): distances and indices of every ref row against the moved src cloud, compute_overlap at
      the radii 0.3 and 0.6, the chamfer distance with raw = ref, and the re-alignment error of the src cloud;
  (b) `scans`: the bundled scan s000004 against s000000 under a fixed pose -- the scalars only.
For every stored query the generator asserts that the nearest and the second nearest support point (a k = 2 query) differ by
more than 1e-9 relative, so the index is decided whatever the rounding of the reference's matmul, and that no nearest distance
lies within 1e-9 relative of a radius, so the overlap counts are decided too; it also checks the reference against the
restatement (tests/nearest_restatement.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
import ref_import  # noqa: E402
sys.path.insert(0, os.path.join(REPO, 'tests'))
import nearest_restatement as R  # noqa: E402

PAIRS = (0, 3)
RADII = (0.3, 0.6)
LIMIT = 1 << 20  # bytes: the largest file that may be committed


def off_pose(T):
    """T with 0.5 degrees about (1, 2, 3) / |.| and 0.2 m along (2, -1, 2) / 3 in front of it."""
    a = np.deg2rad(0.5)
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    D[:3, 3] = 0.2 * np.array([2.0, -1.0, 2.0]) / 3.0
    return D @ T


def main():
    ref_import.install()
    import geotransformer.utils.pointcloud as ref_pc
    import geotransformer.utils.registration as ref_reg
    from scipy.spatial import cKDTree

    class _Tree(cKDTree):  # the reference targets a scipy whose query() still takes n_jobs
        def query(self, x, k=1, n_jobs=None, **kw):
            return super().query(x, k=k, workers=-1 if n_jobs == -1 else 1, **kw)
    ref_pc.cKDTree = _Tree
    ref_reg.get_nearest_neighbor = ref_pc.get_nearest_neighbor  # (registration.py binds the name at import)

    def decided(q64, s64):
        """The smallest relative gap between the nearest and the second nearest support point over all queries."""
        d, _ = cKDTree(s64).query(q64, k=2)
        return float(((d[:, 1] - d[:, 0]) / d[:, 1]).min())

    def scalars(fx, tag, raw, ref, src, gt, est):
        ref64, src64, raw64 = ref.astype(np.float64), src.astype(np.float64), raw.astype(np.float64)
        dist = ref_pc.get_nearest_neighbor(ref64, ref_pc.apply_transform(src64, est))
        for r in RADII:
            assert (np.abs(dist - r) / r).min() > 1e-9, (tag, r)
            o = ref_reg.compute_overlap(ref64, src64, est, r)
            assert o == R.compute_overlap(ref, src, est, r), (tag, r)
            fx[f'{tag}/overlap{r}'] = np.float64(o)
        fx[f'{tag}/chamfer'] = np.float64(ref_reg.compute_modified_chamfer_distance(raw64, ref64, src64, gt, est))
        fx[f'{tag}/rmse'] = np.float64(ref_reg.compute_registration_rmse(src64, gt, est))
        assert abs(fx[f'{tag}/chamfer'] - R.compute_modified_chamfer_distance(raw, ref, src, gt, est)) < 1e-9, tag
        assert abs(fx[f'{tag}/rmse'] - R.compute_registration_rmse(src, gt, est)) < 1e-9, tag
        fx[f'{tag}/gt'], fx[f'{tag}/est'] = gt, est
        print(tag, {k.split('/')[-1]: float(v) for k, v in fx.items() if k.startswith(tag + '/') and np.ndim(v) == 0})

    z = np.load(os.path.join(HERE, 'synthetic_pairs.npz'))
    fx = {'pairs': np.array(PAIRS, np.int64), 'radii': np.array(RADII, np.float64)}
    closest = np.inf
    for p in PAIRS:
        ref, src, T = z[f'ref{p}'], z[f'src{p}'], z[f'T{p}']
        assert ref.dtype == src.dtype == np.float32 and T.dtype == np.float64
        for name, est in (('gt', T), ('off', off_pose(T))):
            tag = f'p{p}/{name}'
            ref64, moved64 = ref.astype(np.float64), ref_pc.apply_transform(src.astype(np.float64), est)
            gap = decided(ref64, moved64)
            assert gap > 1e-9, (tag, gap)
            closest = min(closest, gap)
            dist, idx = ref_pc.get_nearest_neighbor(ref64, moved64, return_index=True)
            d2, want = R.nearest(ref, src, None, est)
            assert np.array_equal(idx, want) and np.abs(dist - np.sqrt(d2)).max() < 1e-9, (tag, 'the restatement and the reference disagree')
            fx[f'{tag}/dist'], fx[f'{tag}/idx'] = dist.astype(np.float64), idx.astype(np.int32)
            scalars(fx, tag, ref, ref, src, T, est)
    s = np.load(os.path.join(HERE, 'scans.npz'))
    gt = np.array([[0.99995, -0.01, 0, 0.1], [0.01, 0.99995, 0, -0.05], [0, 0, 1, 0.02], [0, 0, 0, 1]], np.float64)
    scalars(fx, 'scans', s['s000000'], s['s000000'], s['s000004'], gt, off_pose(gt))
    fx['closest_relative'] = np.float64(closest)
    print('smallest relative gap between nearest and second nearest:', closest)
    path = os.path.join(HERE, 'nearest.npz')
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= LIMIT


if __name__ == '__main__':
    main()
