"""Generates tests/golden/pair_overlap.npz: the reference's get_correspondences and compute_overlap
(geotransformer/utils/registration.py:191-216, on scipy's cKDTree) imported with the shims of ref_import.py, CPU.
Build container only; the fixture travels, the reference not.

Cases:
  (a) pairs 0, 3 and 5 of tests/golden/synthetic_pairs.npz (ref*, src*, T*) at the radii 0.6 and 0.3;
  (b) `two_point`: ref = {(0, 0, 0)}, src = {(0.5, 0, 0)}, r = 0.5 -- the pair lies ON the ball: cKDTree's closed ball lists it,
      compute_overlap's strict comparison does not count it.
The lists are sorted by (i, j) (cKDTree leaves the order inside a row open; this library defines it as ascending j) and stored
as int32.  For every case of (a) the generator asserts that no pair's d2 is within 1e-9 relative of r2 and no nearest distance
within 1e-9 relative of r, so that the reference's own rounding (numpy matmul in float64) cannot decide a row differently from
the restatement (tests/pair_overlap_restatement.py); it records the closest it met.
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
import pair_overlap_restatement as R  # noqa: E402

PAIRS = (0, 3, 5)
RADII = (0.6, 0.3)
LIMIT = 1 << 20  # bytes: the largest file that may be committed


def main():
    ref_import.install()
    np.long = np.int64  # (the reference uses the removed alias)
    import geotransformer.utils.pointcloud as ref_pc
    from geotransformer.utils.registration import compute_overlap, get_correspondences
    from scipy.spatial import cKDTree

    class _Tree(cKDTree):  # the reference targets a scipy whose query() still takes n_jobs
        def query(self, x, k=1, n_jobs=None, **kw):
            return super().query(x, k=k, workers=-1 if n_jobs == -1 else 1, **kw)
    ref_pc.cKDTree = _Tree

    z = np.load(os.path.join(HERE, 'synthetic_pairs.npz'))

    def build(pairs):
        fx = {'pairs': np.array(pairs, np.int64), 'radii': np.array(RADII, np.float64)}
        closest = np.inf
        for p in pairs:
            ref, src, T = z[f'ref{p}'], z[f'src{p}'], z[f'T{p}']
            assert ref.dtype == src.dtype == np.float32 and T.dtype == np.float64
            for r in RADII:
                corr = get_correspondences(ref, src, T, r)
                corr = corr[np.lexsort((corr[:, 1], corr[:, 0]))]
                o_ref = compute_overlap(ref, src, T, r)
                o_src = compute_overlap(src, ref, np.linalg.inv(T), r)  # (recorded only: the src side is checked against the restatement)
                q = R.ball_query(ref, src, T, r)
                r2, s = r * r, R.moved(src, T)
                rel = np.inf  # over ALL pairs (i, j), listed or not
                for i0 in range(0, ref.shape[0], R.BLOCK):
                    rel = min(rel, float((np.abs(R.sq_dists(ref[i0:i0 + R.BLOCK], s) - r2) / r2).min()))
                assert rel > 1e-9, (p, r, rel)
                nearest = np.sqrt(np.concatenate([q['ref_min_d2'], q['src_min_d2']]))
                assert (np.abs(nearest - r) / r).min() > 1e-9, (p, r)
                assert np.array_equal(corr, q['corr']), (p, r, 'the restatement and the reference disagree')
                closest = min(closest, rel)
                fx[f'p{p}/r{r}/corr'] = corr.astype(np.int32)
                fx[f'p{p}/r{r}/overlap'] = np.float64(o_ref)
                fx[f'p{p}/r{r}/overlap_src'] = np.float64(o_src)
                print('pair', p, 'r', r, 'C', len(corr), 'overlap', round(float(o_ref), 3), 'src side', round(float(o_src), 3))
        fx['closest_relative'] = np.float64(closest)
        ref, src = np.zeros((1, 3), np.float32), np.array([[0.5, 0, 0]], np.float32)
        fx['two_point/ref'], fx['two_point/src'], fx['two_point/radius'] = ref, src, np.float64(0.5)
        fx['two_point/corr'] = get_correspondences(ref, src, None, 0.5).astype(np.int32).reshape(-1, 2)
        fx['two_point/overlap'] = np.float64(compute_overlap(ref, src, None, 0.5))
        assert fx['two_point/corr'].tolist() == [[0, 0]] and fx['two_point/overlap'] == 0.0
        print('closest d2 to r2, relative:', closest)
        return fx

    path = os.path.join(HERE, 'pair_overlap.npz')
    for pairs in (PAIRS, PAIRS[:2]):
        np.savez_compressed(path, **build(pairs))
        size = os.path.getsize(path)
        print(path, size, 'bytes', 'pairs', pairs)
        if size <= LIMIT:
            break
    assert os.path.getsize(path) <= LIMIT


if __name__ == '__main__':
    main()
