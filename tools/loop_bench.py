"""Times loop-closure detection (ops.scan_context, ops.scan_context_distance).

  python tools/loop_bench.py [--frames 4541] [--reps 3] [--batch 64] [--cpu] [--cpu-frames 48]
Prints one JSON line per case:
  * descriptors: a batch of synthetic clouds of 16 384 points (a down-sampled scan) and of 122 880 points (a raw scan), ms per batch
    and per scan, device time between two events;
  * search: one exhaustive search of --frames seeded random descriptors (about half the bins empty) against themselves with
    exclude_recent = 50, in the best-only mode; eligible pairs, pairs/s and the rate of the useful multiply-adds (pairs x 60 shifts x
    1 200 products) as a fraction of the fp32 vector peak (157.3 TFLOP/s = 78.65e12 multiply-adds/s);
  * with --cpu: the float64 numpy restatement (tests/scan_context_restatement.py) on --cpu-frames descriptors, every pair, and its
    pairs/s beside the GPU's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

PEAK_FMA = 157.3e12 / 2  # fp32 vector multiply-adds per second
N_RINGS, N_SECTORS = 20, 60


def timed(fn, reps):
    """Median device time in ms of fn() between two events, after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def synthetic_cloud(n, seed):
    """n points of a ground plane with boxes on it, out to 90 m (some beyond the range limit)."""
    rng = np.random.default_rng(seed)
    r = 90.0 * np.sqrt(rng.random(n))
    th = rng.uniform(0, 2 * np.pi, n)
    z = -1.7 + 0.05 * rng.standard_normal(n) + (rng.random(n) < 0.3) * rng.uniform(0, 4.0, n)
    return np.stack([r * np.cos(th), r * np.sin(th), z, rng.random(n)], 1).astype(np.float32)


def random_descriptors(n, seed):
    rng = np.random.default_rng(seed)
    D = rng.uniform(-0.7, 3.0, (n, N_RINGS, N_SECTORS)).astype(np.float32)
    return np.where(rng.random(D.shape) < 0.5, D, np.float32(0))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=4541, help='descriptors of the search (default 4541: KITTI sequence 00)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64, help='clouds per descriptor call')
    ap.add_argument('--cpu', action='store_true', help='also time the numpy restatement')
    ap.add_argument('--cpu-frames', type=int, default=48)
    a = ap.parse_args(argv)
    import torch
    from rdmnet_amd import ops
    assert torch.cuda.is_available(), 'loop_bench needs a GPU'
    for points in (16384, 122880):
        clouds = torch.from_numpy(np.concatenate([synthetic_cloud(points, s) for s in range(4)])).cuda()
        clouds = clouds.repeat((a.batch + 3) // 4, 1)[:a.batch * points]
        offsets = torch.arange(a.batch + 1, dtype=torch.int64).cuda() * points
        ms, desc = timed(lambda: ops.scan_context(clouds, offsets), a.reps)
        print(json.dumps({'case': 'descriptors', 'points': points, 'batch': a.batch, 'ms_per_batch': round(ms, 4),
                          'ms_per_scan': round(ms / a.batch, 5), 'GB_per_s': round(clouds.numel() * 4 / ms / 1e6, 1),
                          'nonzero_bins': float((desc[0] != 0).float().mean())}))
    n = a.frames
    desc = torch.from_numpy(random_descriptors(n, 1)).cuda()
    ms, res = timed(lambda: ops.scan_context_distance(desc, desc, exclude_recent=50), a.reps)
    pairs = max(n - 50, 0) * (max(n - 50, 0) + 1) // 2
    fma = pairs * N_SECTORS * N_RINGS * N_SECTORS
    print(json.dumps({'case': 'search', 'frames': n, 'exclude_recent': 50, 'ms': round(ms, 3), 'eligible_pairs': pairs,
                      'pairs_per_s': round(pairs / ms * 1e3), 'useful_fma': fma, 'fma_per_s': round(fma / ms * 1e3),
                      'fraction_of_fp32_vector_peak': round(fma / ms * 1e3 / PEAK_FMA, 4),
                      'queries_with_a_candidate': int((res.index >= 0).sum())}))
    if a.cpu:
        import scan_context_restatement as SC
        m = min(a.cpu_frames, n)
        host = desc[:m].cpu().numpy()
        t0 = time.perf_counter()
        d64, _, _ = SC.distance_matrix(host, host)
        cpu_s = time.perf_counter() - t0
        gms, full = timed(lambda: ops.scan_context_distance(desc[:m], desc[:m], exclude_recent=-1, full=True), a.reps)
        err = float(np.abs(full.distances.cpu().numpy().astype(np.float64) - d64).max())
        print(json.dumps({'case': 'cpu restatement', 'frames': m, 'pairs': m * m, 'cpu_s': round(cpu_s, 3),
                          'cpu_pairs_per_s': round(m * m / cpu_s), 'gpu_pairs_per_s_at_frames': round(pairs / ms * 1e3),
                          'gpu_ms_same_problem_full_matrix': round(gms, 4), 'max_abs_difference': err}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
