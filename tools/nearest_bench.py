"""Times the exact nearest-neighbour query (rdm_nearest, ops.get_nearest_neighbor) on a 2 x 16 k synthetic pair
(tests/golden/synthetic_pairs.npz, pair 0 under its ground-truth transform) and on a raw-shaped synthetic pair (2 x ~120 k
points, tools/icp_bench.py's generator), both directions at the automatic cell, and, for comparison, scipy's cKDTree k = 1
query -- what the reference's get_nearest_neighbor calls -- on the same float64 points with 16 host threads.  The src_to_ref
side is also timed as rdm_information_matrix (ops.information_matrix at 0.6 m with the correspondence set: the same search plus the
reduction and the compaction) and, with --cpu, as its float64 host restatement on the cKDTree query.  --ball adds the ball
query on the same clouds (rdm_ball_count / rdm_ball_fill): ops.pair_overlap (the count pass) and ops.get_correspondences (count and
list) at 0.6 m.

  python tools/nearest_bench.py [--reps 5] [--cpu] [--ball]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/nearest_bench.py --reps 1      # per-kernel times, a run of its own
Prints one JSON line per pair: sizes, the share of rows that took the exact sweep, GPU ms per call (median), cKDTree ms (--cpu)."""
RADIUS = 0.6  # cfg.fine_matching.acceptance_radius
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]


def cases():
    import icp_bench
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'synthetic_pairs.npz'))
    yield 'synthetic_pair0', z['ref0'], z['src0'], z['T0']
    src, tgt, init = icp_bench.pair()
    yield 'raw_shaped', tgt, src, init


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', action='store_true', help="also time scipy's cKDTree (build + k = 1 query, 16 threads)")
    ap.add_argument('--ball', action='store_true', help='also time the ball query: pair_overlap and get_correspondences at 0.6 m')
    a = ap.parse_args()
    import torch
    from rdmnet_amd import ops
    for name, ref, src, T in cases():
        r, s = torch.from_numpy(ref).cuda(), torch.from_numpy(src).cuda()
        out = {'case': name, 'n_ref': len(ref), 'n_src': len(src)}
        for side, args in (('ref_to_src', (r, s, None, T)), ('src_to_ref', (s, r, T, None))):
            _, d2, totals = ops._nearest(*args)  # warm-up (workspace, code objects)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ops._nearest(*args)  # (ends with the call's read-back)
                times.append((time.perf_counter() - t0) * 1e3)
            out[side] = {'gpu_ms': float(np.median(times)), 'gpu_ms_all': times, 'swept_share': totals[3] / max(args[0].shape[0], 1),
                         'mean_distance': totals[0] / max(args[0].shape[0], 1)}
        ops.information_matrix(s, r, RADIUS, T, return_correspondences=True)  # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            info, corr = ops.information_matrix(s, r, RADIUS, T, return_correspondences=True)  # (ends with the call's read-back)
            times.append((time.perf_counter() - t0) * 1e3)
        out['information'] = {'gpu_ms': float(np.median(times)), 'gpu_ms_all': times, 'C': int(corr.shape[0]),
                              'over_nearest': float(np.median(times)) / out['src_to_ref']['gpu_ms']}
        if a.ball:
            for key, call in (('pair_overlap', lambda: ops.pair_overlap(r, s, T, RADIUS)),
                              ('get_correspondences', lambda: ops.get_correspondences(r, s, T, RADIUS))):
                res = call()  # warm-up
                torch.cuda.synchronize()
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()  # (the list is filled after the count's read-back)
                    times.append((time.perf_counter() - t0) * 1e3)
                out[key] = {'gpu_ms': float(np.median(times)), 'gpu_ms_all': times,
                            'C': int(res[2] if key == 'pair_overlap' else res.shape[0])}
        if a.cpu:
            import nearest_restatement as R
            from scipy.spatial import cKDTree
            q64, s64 = ref.astype(np.float64), R.moved(src, T)
            t0 = time.perf_counter()
            d, _ = cKDTree(s64).query(q64, k=1, workers=16)
            out['ckdtree_ref_to_src_ms'] = (time.perf_counter() - t0) * 1e3
            out['ckdtree_vs_gpu_max_abs'] = float(np.abs(d - torch.sqrt(ops._nearest(r, s, None, T)[1]).cpu().numpy()).max())
            t0 = time.perf_counter()  # the information matrix on the host: tree, query, the rows under the radius, the sums
            m64 = R.moved(src, T)
            d, j = cKDTree(q64).query(m64, k=1, workers=16)
            p = q64[j[d < RADIUS]]
            M, sp = p.T @ p, p.sum(axis=0)
            host = np.zeros((6, 6))
            host[:3, :3] = np.trace(M) * np.eye(3) - M
            host[:3, 3:] = np.array([[0, -sp[2], sp[1]], [sp[2], 0, -sp[0]], [-sp[1], sp[0], 0]])
            host[3:, :3] = host[:3, 3:].T
            host[3:, 3:] = len(p) * np.eye(3)
            out['ckdtree_information_ms'] = (time.perf_counter() - t0) * 1e3
            out['ckdtree_information_C'] = int(len(p))
            out['ckdtree_information_max_rel'] = float(np.abs(host - info.numpy()).max() / np.abs(host).max())
        print(json.dumps(out))


if __name__ == '__main__':
    main()
