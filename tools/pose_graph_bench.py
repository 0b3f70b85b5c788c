"""Times ops.pose_graph_optimize (rdm_pose_graph_optimize) on a KITTI-shaped pose graph -- a drive of about 500 scans with
odometry edges, noisy loop closures and a line process -- alone and as a batch of 11 such graphs, and, with --cpu, the host
for comparison: the restatement's dense solve (tests/pose_graph_restatement.py, numpy on the threads OMP_NUM_THREADS gives it)
and, where scipy is importable, the same damped Gauss-Newton iteration with a sparse direct solve (scipy.sparse.linalg.spsolve).

  python tools/pose_graph_bench.py [--nodes 500] [--loops 40] [--batch 11] [--reps 3] [--cpu] [--preconditioner chain]
                                     [--linear-solver direct]
Prints one JSON line: sizes, GPU ms per call (median; a call ends with its read-back), outer iterations, PCG iterations per outer
iteration, and the host's ms per solve.  --preconditioner (block_jacobi | chain) is passed to ops.pose_graph_optimize and named in
the output; without the flag the call and the output are what they were.  --linear-solver (pcg | direct) likewise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

MU = 1.0
TOL = dict(gradient_tolerance=1e-6, cost_tolerance=1e-9, max_iterations=30)  # (Gauss-Newton gains slowly on a 500-scan chain)


def graph(n, loops, seed):
    import pose_graph_cases as cases
    rng = np.random.default_rng(seed)
    truth = cases.trajectory_truth(rng, n)
    odo = [(i + 1, i) for i in range(n - 1)]
    loop = [(int(s), int(s) - int(rng.integers(50, 200))) for s in rng.choice(np.arange(200, n), size=loops, replace=False)]
    c = cases.make(truth, odo + loop, rng, start_angle=0.0, start_distance=0.0, noise_angle=0.01, noise_distance=0.05,
                   uncertain=[0] * len(odo) + [1] * len(loop))
    c['nodes'] = cases.chained_start(c)
    return c


def sparse_solve(R, c, max_iterations=TOL['max_iterations']):
    """The restatement's iteration with scipy's sparse direct solve in place of np.linalg.solve."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    X = c['nodes'].copy()
    args = (c['edges'], c['transforms'], c['informations'], c['uncertain'], MU)
    n = len(X)
    F = R.cost(X, *args)
    lam = R.LAMBDA0
    steps = 0
    for it in range(max_iterations):
        steps = it + 1
        rows, cols, vals = [], [], []
        b = np.zeros(6 * n)
        diag = np.zeros((n, 6, 6))
        for e, (s, t) in enumerate(c['edges']):
            r, A, B = R.jacobians(X[s], X[t], c['transforms'][e])
            L = R.sym(c['informations'][e])
            l = R.weight(float(r @ L @ r), MU, c['uncertain'][e])
            for (i, Ji), (j, Jj) in (((s, A), (s, A)), ((s, A), (t, B)), ((t, B), (s, A)), ((t, B), (t, B))):
                blk = l * (Ji.T @ L @ Jj)
                rr, cc = np.meshgrid(np.arange(6 * i, 6 * i + 6), np.arange(6 * j, 6 * j + 6), indexing='ij')
                rows.append(rr.ravel()), cols.append(cc.ravel()), vals.append(blk.ravel())
                if i == j:
                    diag[i] += blk
            b[6 * s:6 * s + 6] += l * (A.T @ L @ r)
            b[6 * t:6 * t + 6] += l * (B.T @ L @ r)
        if np.abs(2 * b[6:]).max() <= TOL['gradient_tolerance']:
            break
        H = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))
        D = sp.block_diag(list(diag[1:]), format='csr')
        d = spl.spsolve((H[6:, 6:] + lam * D).tocsc(), -b[6:])
        Xc = X.copy()
        for i in range(1, n):
            Xc[i] = R.retract(X[i], d[6 * (i - 1):6 * i])
        Fc = R.cost(Xc, *args)
        if Fc <= F:
            rel = (F - Fc) / F if F > 0 else 0.0
            X, F, lam = Xc, Fc, max(lam * R.LAMBDA_DOWN, R.LAMBDA_MIN)
            if rel <= TOL['cost_tolerance']:
                break
        else:
            lam *= R.LAMBDA_UP
    return F, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=500)
    ap.add_argument('--loops', type=int, default=40)
    ap.add_argument('--batch', type=int, default=11)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu', action='store_true', help='also time the host: the dense restatement and, with scipy, a sparse solve')
    ap.add_argument('--preconditioner', choices=('block_jacobi', 'chain'), default=None)
    ap.add_argument('--linear-solver', choices=('pcg', 'direct'), default=None)
    a = ap.parse_args()
    import torch
    from rdmnet_amd import ops
    import pose_graph_restatement as R
    graphs = [graph(a.nodes, a.loops, 40 + k) for k in range(a.batch)]
    out = {'nodes': a.nodes, 'edges': len(graphs[0]['edges']), 'batch': a.batch, 'line_process_weight': MU}
    extra = {}
    if a.preconditioner is not None:
        out['preconditioner'] = a.preconditioner
        extra['preconditioner'] = a.preconditioner
    if a.linear_solver is not None:
        out['linear_solver'] = a.linear_solver
        extra['linear_solver'] = a.linear_solver

    def run(gs):
        noff = np.cumsum([0] + [len(g['nodes']) for g in gs])
        eoff = np.cumsum([0] + [len(g['edges']) for g in gs])
        cat = {k: np.concatenate([g[k] for g in gs]) for k in ('nodes', 'edges', 'transforms', 'informations', 'uncertain')}
        dev = {k: torch.from_numpy(cat[k]).cuda() for k in ('nodes', 'transforms', 'informations')}
        call = lambda: ops.pose_graph_optimize(dev['nodes'], cat['edges'], dev['transforms'], dev['informations'], cat['uncertain'],
                                               line_process_weight=MU, graph_node_offsets=noff, graph_edge_offsets=eoff, **TOL, **extra)
        res = call()  # warm-up (workspace, code objects)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = call()
            times.append((time.perf_counter() - t0) * 1e3)
        return {'gpu_ms': float(np.median(times)), 'gpu_ms_all': times, 'iterations': res.iterations.tolist(),
                'pcg_per_iteration': (res.pcg_iterations / np.maximum(res.iterations, 1)).round(1).tolist(),
                'stop': res.stop_reasons, 'cost': [res.initial_cost.tolist(), res.final_cost.tolist()],
                'pruned': int(res.pruned.sum())}

    out['one_graph'] = run(graphs[:1])
    out['batch_of_graphs'] = run(graphs)
    if a.cpu:
        c = graphs[0]
        t0 = time.perf_counter()
        res = R.optimize(c['nodes'], c['edges'], c['transforms'], c['informations'], c['uncertain'], MU, **TOL)
        out['host_dense'] = {'ms': (time.perf_counter() - t0) * 1e3, 'iterations': res['iterations'], 'cost': res['cost'],
                             'threads': os.environ.get('OMP_NUM_THREADS')}
        try:
            import scipy  # noqa: F401
        except ImportError:
            out['host_sparse'] = 'scipy is not importable'
        else:
            t0 = time.perf_counter()
            F, its = sparse_solve(R, c)
            out['host_sparse'] = {'ms': (time.perf_counter() - t0) * 1e3, 'iterations': its, 'cost': F}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
