"""Times ops.robust_registration (maximum clique + GNC-TLS + translation voting) per call at C = 250, 1000 and 5000
correspondences, at 10 % and at 50 % planted inliers (tests/robust_restatement.make_fixture, noise bound 0.01), with
ops.ransac_correspondences (50 000 iterations, 0.3 m) on the same rows beside it and, with --cpu, the float64 restatement
(C <= 1000: networkx enumerates every maximal clique).

  python tools/robust_bench.py [--reps 5] [--cpu] [--node-rate]
Prints one JSON line per case.  --node-rate measures the clique search's speed instead: C = 5471 random rows (the largest pair of
tests/golden/eval_pairs.npz has that many) in a box that makes the graph dense, so that every subproblem runs out of its budget;
the difference of two budgets gives search nodes per second, per search wavefront and in total (DESIGN.md section 7 derives the
default budget from it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def timed(fn, reps):
    import torch
    fn()  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), out


def search_waves(C, maxcore, pool_bytes=256 << 20, max_waves=1024):
    """The number of search wavefronts robust.hip plans (greedy_kernel): pool / ((max core + 2) levels of W + 1 words)."""
    W = (C + 63) // 64
    one = (C + 2) * (W + 1)
    pool_words = one * max(1, min(max_waves, pool_bytes // (one * 8)))
    return int(max(1, min(max_waves, pool_words // ((maxcore + 2) * (W + 1)))))


def node_rate(reps):
    import torch
    from rdmnet_amd import ops
    C = 5471
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.uniform(-2, 2, (C, 3)).astype(np.float32)).cuda()
    ref = torch.from_numpy(rng.uniform(-2, 2, (C, 3)).astype(np.float32)).cuda()
    out = {'C': C}
    ms = {}
    for budget in (500, 2500):
        ms[budget], res = timed(lambda: ops.robust_registration(src, ref, noise_bound=0.3, max_clique_nodes=budget,
                                                                return_graph=True), reps)
        out[f'ms_budget_{budget}'] = ms[budget]
        out.update(density=res.edges / (C * (C - 1) / 2), exact=res.exact, K=res.num_selected, max_core=int(res.core.max()))
    waves = search_waves(C, out['max_core'])
    total = C * (2500 - 500) / ((ms[2500] - ms[500]) * 1e-3)  # every subproblem uses its whole budget (exact = 0)
    out.update(search_waves=waves, nodes_per_second=total, nodes_per_second_per_wave=total / waves,
               budget_for_one_second=total / C)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', action='store_true', help='also time the float64 restatement (C <= 1000)')
    ap.add_argument('--node-rate', action='store_true', help='measure the clique search: nodes per second at C = 5471')
    a = ap.parse_args()
    import torch
    import robust_restatement as RR
    from rdmnet_amd import ops
    if a.node_rate:
        return node_rate(a.reps)
    for C in (250, 1000, 5000):
        for frac in (0.1, 0.5):
            n_in = int(C * frac)
            src, ref, rows, poses = RR.make_fixture(C, n_in, 0.01, seed=C)
            s, r = torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda()
            ms, res = timed(lambda: ops.robust_registration(s, r, noise_bound=0.01), a.reps)
            rms, rres = timed(lambda: ops.ransac_correspondences(s, r, 0.3, 4, 50000)[0].cpu(), a.reps)
            rre, rte = RR.pose_error(res.transformation, poses[0])
            rr2, rt2 = RR.pose_error(rres.numpy().astype(np.float64), poses[0])
            out = {'C': C, 'inliers': n_in, 'robust_ms': ms, 'K': res.num_selected, 'exact': res.exact, 'iterations': res.iterations,
                   'planted_rows_found': bool(np.array_equal(res.selected, rows[0])), 'rre_deg': rre, 'rte_m': rte,
                   'ransac_ms': rms, 'ransac_rre_deg': rr2, 'ransac_rte_m': rt2}
            if a.cpu and C <= 1000:
                t0 = time.perf_counter()
                want = RR.robust_registration(src, ref, 0.01)
                out.update(cpu_ms=(time.perf_counter() - t0) * 1e3, cpu_vs_gpu_max_abs=float(np.abs(want.transform - res.transformation).max()))
            print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
