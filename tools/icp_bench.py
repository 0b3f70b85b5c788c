"""Times the GPU point-to-point ICP on a synthetic raw pair (2 x ~120 k points, 0.5 m, the pair generation's settings)
and, for comparison, the float64 restatement of tests/icp_restatement.py on the host.

  python tools/icp_bench.py [--reps 3] [--cpu]
Prints one JSON line: updates to convergence, total ms, ms per evaluation (GPU), and the restatement's total (--cpu)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def pair(seed=2):
    from rdmnet_amd import synthetic
    rng = np.random.default_rng(seed)
    boxes = synthetic._make_scene(rng)
    tgt = synthetic._scan(boxes, (0.0, 0.0), 0.0, 2048, rng)
    src = synthetic._scan(boxes, (1.2, 0.1), np.deg2rad(0.4), 2048, rng)
    a, b = np.deg2rad(0.4 + 0.3), np.deg2rad(0.0)
    init = np.eye(4)  # the true motion, off by 0.3 deg and a few cm (a drifted odometry pose)
    init[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    init[:3, 3] = [1.2 + 0.08, 0.1 - 0.05, 0.03]
    return src, tgt, init


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu', action='store_true', help='also time the float64 restatement (16 host threads)')
    ap.add_argument('--max-iteration', type=int, default=5000)
    a = ap.parse_args()
    import torch
    from rdmnet_amd import ops
    src, tgt, init = pair()
    s, t = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    ops.icp_point_to_point(s, t, 0.5, init=init, max_iteration=a.max_iteration)  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    times, res = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = ops.icp_point_to_point(s, t, 0.5, init=init, max_iteration=a.max_iteration)
        times.append((time.perf_counter() - t0) * 1e3)
    total = float(np.median(times))
    out = {'n_source': len(src), 'n_target': len(tgt), 'updates': res.iterations, 'fitness': res.fitness,
           'rmse': res.inlier_rmse, 'gpu_total_ms': total, 'gpu_ms_per_evaluation': total / (res.iterations + 1),
           'gpu_totals_ms': times}
    if a.cpu:
        import icp_restatement as ir
        t0 = time.perf_counter()
        T, fit, rmse, n, it = ir.icp(src, tgt, 0.5, init=init, max_iteration=a.max_iteration)
        out.update(cpu_total_ms=(time.perf_counter() - t0) * 1e3, cpu_updates=it,
                   cpu_vs_gpu_max_abs=float(np.abs(T - res.transformation).max()))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
