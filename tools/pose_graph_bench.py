"""Times ops.pose_graph_optimize (rdm_pose_graph_optimize) on a KITTI-shaped pose graph -- a drive of about 500 scans with
odometry edges, noisy loop closures and a line process -- alone and as a batch of 11 such graphs, and, with --cpu, the host
for comparison: the restatement's dense solve (tests/pose_graph_restatement.py, numpy on the threads OMP_NUM_THREADS gives it)
and, where scipy is importable, the same damped Gauss-Newton iteration with a sparse direct solve (scipy.sparse.linalg.spsolve).

  python tools/pose_graph_bench.py [--nodes 500] [--loops 40] [--batch 11] [--reps 3] [--cpu] [--preconditioner chain]
                                     [--linear-solver direct] [--marginals] [--consistency] [--digest host | gpu]
With --digest (and nothing else): no timing, one sha1 line per result of the library's host entry points (host: no GPU needed, see
digest_host()) or of the GPU solves of the test graphs (gpu, see digest_gpu()), for comparing the bits of two builds of the library
(RDM_LIB_PATH).  Otherwise prints one JSON line: sizes, GPU ms per call (median; a call ends with its read-back), outer iterations, PCG iterations per outer
iteration, and the host's ms per solve.  --preconditioner (block_jacobi | chain) is passed to ops.pose_graph_optimize and named in
the output; without the flag the call and the output are what they were.  --linear-solver (pcg | direct) likewise.  --marginals
also times ops.pose_graph_marginals (rdm_pose_graph_marginals) at the optimised poses with the final weights, pruned edges at 0,
beside the optimise call of the same run -- ms per call, its ratio to the optimise call, and for the single graph how the run
sweep's wavefronts spent their time (rdm_dbg_pose_graph_marginals_ticks: the columns' products, the butterflies, the nodes' steps) --
and, with --cpu, np.linalg.inv on the same graph's dense H.  --consistency (which implies --marginals, whose figures stay beside it)
also times ops.pose_graph_consistency (rdm_pose_graph_consistency) on the same graph, poses and weights, once with every graph's loop
edges as the pairs (their own transforms and informations) and once with 4096 seeded random pairs per graph (the current relative
poses, no informations) -- ms per call, its ratio to the marginals call, the distinct column nodes -- and, with --cpu, the dense
route beside it: np.linalg.inv of H (the figure above) plus reading the pairs' blocks out of it."""
import argparse
import hashlib
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


def sha1_line(what, arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f'{h.hexdigest()}  {what}', flush=True)


def digest_host():
    """One `sha1  what` line over the raw bytes that the library's host entry points return (no GPU): the chain solve on
    chain_system of tests/test_pose_graph_chain.py, the direct solve and the separator on every shape of
    tests/test_pose_graph_direct.py, the edge terms and the retraction on cases.noisy(), and the three workspace sizes."""
    import ctypes
    import pose_graph_cases as cases
    import test_pose_graph_chain as tc
    import test_pose_graph_direct as td
    from rdmnet_amd import _lib
    L = _lib.lib()
    for n in (1, 2, 3, 50, 300):
        diag, off, _ = tc.chain_system(n, seed=100 + n)
        rhs = np.ascontiguousarray(np.random.default_rng(n).normal(size=(n, 6)) * 100.0)
        rc, out = tc.chain_host(diag, off, rhs)
        sha1_line(f'chain_host n {n} rc {rc}', [out])
    for name, (n, chords, _) in td.SHAPES.items():
        edges, diag, off, rhs = td.random_system(n, chords, seed=200 + n + len(chords))
        rc, out = td.direct_host(n, edges, diag, off, rhs)
        sha1_line(f'direct_host {name} rc {rc}', [out])
        size, sep = td.separator(n, edges)
        sha1_line(f'separator_host {name} size {size}', [sep])
    c = cases.noisy()
    terms = np.zeros((len(c['edges']), 128))
    for e, (s, t) in enumerate(c['edges'].tolist()):
        Xs, Xt, T, Lm = (np.ascontiguousarray(a, dtype=np.float64) for a in (c['nodes'][s], c['nodes'][t], c['transforms'][e],
                                                                              c['informations'][e]))
        rc = L.rdm_pose_graph_edge_terms_host(Xs.ctypes.data, Xt.ctypes.data, T.ctypes.data, Lm.ctypes.data, ctypes.c_double(MU),
                                              int(c['uncertain'][e]), terms[e].ctypes.data)
        assert rc == 0
    sha1_line('edge_terms_host noisy', [terms])
    rng = np.random.default_rng(0)
    moved = np.zeros_like(c['nodes'])
    for i, X in enumerate(c['nodes']):
        d = np.ascontiguousarray(rng.normal(size=6) * (0.01 if i % 2 else 1.0))  # (both branches of the series)
        assert L.rdm_pose_graph_retract_host(np.ascontiguousarray(X).ctypes.data, d.ctypes.data, moved[i].ctypes.data) == 0
    sha1_line('retract_host noisy', [moved])
    for G, N, E in ((1, 1, 0), (1, 2, 1), (3, 700, 760), (11, 5500, 5929)):
        # G chains of N / G nodes (the first ones one longer), the other edges as chords (s, s - 2 - k) dealt out in turn
        sizes = [N // G + (1 if g < N % G else 0) for g in range(G)]
        extra = [(E - (N - G)) // G + (1 if g < (E - (N - G)) % G else 0) for g in range(G)]
        edges = [[(i + 1, i) for i in range(n - 1)] + [(n - 1 - 3 * k, n - 3 - 4 * k) for k in range(x)] for n, x in zip(sizes, extra)]
        noff = np.cumsum([0] + sizes).astype(np.int64)
        eoff = np.cumsum([0] + [len(e) for e in edges]).astype(np.int64)
        assert noff[-1] == N and eoff[-1] == E
        ed = np.array([p for e in edges for p in e], np.int64).reshape(-1, 2)
        got = [L.rdm_pose_graph_workspace_bytes(G, N, E)]
        got += [L.rdm_pose_graph_workspace_bytes_pc(G, N, E, pre) for pre in (0, 1)]
        got += [L.rdm_pose_graph_workspace_bytes_ls(G, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data, pre, solver)
                for pre in (0, 1) for solver in (0, 1)]
        assert all(v > 0 for v in got), got
        sha1_line(f'workspace_bytes G {G} N {N} E {E}', [np.array(got, np.uint64)])
    # (the marginals' lines come last: the lines above are what they were)
    import test_pose_graph_marginals as tm
    for name, (n, chords, _) in tm.SHAPES.items():
        edges, diag, off, _ = td.random_system(n, chords, seed=300 + n + len(chords))
        rc, out = tm.marginals_host(n, edges, diag, off)
        sha1_line(f'marginals_host {name} rc {rc}', [out])
    diag, off = tm.system(c, np.ones(len(c['edges'])))
    rc, out = tm.marginals_host(len(c['nodes']), c['edges'], diag, off)
    sha1_line(f'marginals_host noisy rc {rc}', [out])


def digest_gpu():
    """One `sha1  what` line over nodes, weights, pruned and the report of ops.pose_graph_optimize for the graphs of the GPU tests
    (every consistent case, noisy() with and without a gross edge, the 150-scan drive with and without a line process, the six-node
    case of mixed directions and doubled pairs, and the one-node, two-node, 60-node batch), each under block-Jacobi PCG, chain PCG
    and the direct solve, alone and as one batch of all of them.  Two libraries (RDM_LIB_PATH) compute the same bits iff they print
    the same lines."""
    import torch
    import pose_graph_cases as cases
    import test_pose_graph_chain_gpu as tg
    import test_pose_graph_direct_gpu as tdg
    from rdmnet_amd import ops
    ten = dict(max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0)
    tol = dict(gradient_tolerance=1e-9, cost_tolerance=1e-12)
    one = {k: cases.consistent('pair')[k][:1] if k == 'nodes' else cases.consistent('pair')[k][:0] for k in tg.KEYS}
    drive = tdg.drive()
    runs = [(name, [cases.consistent(name)], ten) for name in cases.CONSISTENT]
    runs += [('noisy', [cases.noisy()], dict(line_process_weight=MU, **tol)),
             ('noisy gross 3', [cases.noisy(gross=3)], dict(line_process_weight=MU, **tol)),
             ('drive 150', [drive], dict(max_iterations=30, **tol)),
             ('drive 150 mu', [drive], dict(line_process_weight=MU, max_iterations=30, **tol)),
             ('six nodes', [tg.six_node_case()], ten),
             ('sizes 1, 2, 60', [one, cases.consistent('pair'), cases.noisy()], tol)]
    everything = [g for name, graphs, _ in runs if name != 'drive 150 mu' for g in graphs]
    runs += [('all', everything, dict(max_iterations=30, **tol)), ('all mu', everything, dict(line_process_weight=MU, max_iterations=30, **tol))]
    solvers = (('block_jacobi', dict(preconditioner='block_jacobi')), ('chain', dict(preconditioner='chain')),
               ('direct', dict(linear_solver='direct')))
    fields = ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping', 'gradient_max')
    for name, graphs, kw in runs:
        noff = np.cumsum([0] + [len(g['nodes']) for g in graphs])
        eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
        cat = {k: np.concatenate([g[k] for g in graphs]) for k in tg.KEYS}
        for solver, extra in solvers:
            res = ops.pose_graph_optimize(torch.from_numpy(cat['nodes']).cuda(), cat['edges'], torch.from_numpy(cat['transforms']).cuda(),
                                          torch.from_numpy(cat['informations']).cuda(), cat['uncertain'], graph_node_offsets=noff,
                                          graph_edge_offsets=eoff, **kw, **extra)
            nodes, weights, pruned = res.nodes.cpu().numpy(), res.weights.cpu().numpy(), res.pruned.cpu().numpy()
            for k in range(len(graphs)):
                report = np.array([getattr(res, f)[k] for f in fields], np.float64)
                sha1_line(f'{name} graph {k} {solver} steps {res.iterations[k]} pcg {res.pcg_iterations[k]}',
                          [nodes[noff[k]:noff[k + 1]], weights[eoff[k]:eoff[k + 1]], pruned[eoff[k]:eoff[k + 1]], report])
    # (the marginals' lines come last: the lines above are what they were)
    import pose_graph_marginals_restatement as M
    for name in M.GRAPHS:
        c, w, _ = M.graph(name)
        res = ops.pose_graph_marginals(torch.from_numpy(c['nodes']).cuda(), c['edges'], torch.from_numpy(c['transforms']).cuda(),
                                       torch.from_numpy(c['informations']).cuda(), torch.from_numpy(w).cuda())
        sha1_line(f'marginals {name} status {res.status[0]} separator {res.separator[0]}', [res.covariances.cpu().numpy()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--digest', choices=('host', 'gpu'), default=None,
                    help='no timing: the sha1 lines of the host entry points (no GPU needed) or of the GPU solves')
    ap.add_argument('--nodes', type=int, default=500)
    ap.add_argument('--loops', type=int, default=40)
    ap.add_argument('--batch', type=int, default=11)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu', action='store_true', help='also time the host: the dense restatement and, with scipy, a sparse solve')
    ap.add_argument('--preconditioner', choices=('block_jacobi', 'chain'), default=None)
    ap.add_argument('--linear-solver', choices=('pcg', 'direct'), default=None)
    ap.add_argument('--marginals', action='store_true', help='also time ops.pose_graph_marginals at the optimised poses')
    ap.add_argument('--consistency', action='store_true',
                    help='also time ops.pose_graph_consistency there: the loop edges as pairs, and 4096 random pairs per graph')
    a = ap.parse_args()
    a.marginals = a.marginals or a.consistency
    if a.digest is not None:
        return digest_host() if a.digest == 'host' else digest_gpu()
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
        row = {'gpu_ms': float(np.median(times)), 'gpu_ms_all': times, 'iterations': res.iterations.tolist(),
               'pcg_per_iteration': (res.pcg_iterations / np.maximum(res.iterations, 1)).round(1).tolist(),
               'stop': res.stop_reasons, 'cost': [res.initial_cost.tolist(), res.final_cost.tolist()],
               'pruned': int(res.pruned.sum())}
        if a.marginals:
            w = torch.where(res.pruned, torch.zeros_like(res.weights), res.weights)
            marg = lambda: ops.pose_graph_marginals(res.nodes, cat['edges'], dev['transforms'], dev['informations'], w,
                                                    graph_node_offsets=noff, graph_edge_offsets=eoff)
            m = marg()  # warm-up
            torch.cuda.synchronize()
            mt = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                m = marg()
                mt.append((time.perf_counter() - t0) * 1e3)
            sigma = torch.sqrt(torch.diagonal(m.covariances[:, 3:, 3:], dim1=1, dim2=2).sum(1))
            row.update({'marginals_ms': float(np.median(mt)), 'marginals_ms_all': mt, 'marginals_per_optimize': float(np.median(mt)) / row['gpu_ms'],
                        'marginals_status': m.status.tolist(), 'separator': m.separator.tolist(),
                        'position_sigma_max_m': float(sigma.max())})
            if len(gs) == 1:  # the run sweep's phase clocks: 3 ticks of 10 ns per run
                from rdmnet_amd import _lib
                ticks = torch.zeros(3 * len(cat['nodes']), dtype=torch.int64, device='cuda')
                _lib.lib().rdm_dbg_pose_graph_marginals_ticks(ticks.data_ptr())
                try:
                    marg()
                    torch.cuda.synchronize()
                finally:
                    _lib.lib().rdm_dbg_pose_graph_marginals_ticks(0)
                t = ticks.cpu().numpy().reshape(-1, 3)
                t = t[t.sum(1) > 0] * 1e-2  # microseconds
                row['sweep_runs'] = len(t)
                row['sweep_us_longest_run'] = dict(zip(('columns', 'butterflies', 'node_steps'), t[np.argmax(t.sum(1))].round(1).tolist()))
                row['sweep_us_all_runs'] = dict(zip(('columns', 'butterflies', 'node_steps'), t.sum(0).round(1).tolist()))
        if a.consistency:
            import pose_graph_consistency_restatement as C
            X = res.nodes.cpu().numpy()
            rng = np.random.default_rng(7)
            loops, rand = [], []
            for k, g in enumerate(gs):
                unc = np.nonzero(g['uncertain'])[0]
                loops.append((g['edges'][unc], g['transforms'][unc], g['informations'][unc]))
                pr = rng.integers(0, len(g['nodes']), size=(3 * 4096, 2))
                pr = pr[pr[:, 0] != pr[:, 1]][:4096]
                Xg = X[noff[k]:noff[k + 1]]
                rand.append((pr, np.stack([C.current_transform(Xg[s], Xg[t]) for s, t in pr]), None))
            for name, sets in (('loop_edges', loops), ('random_4096', rand)):
                poff = np.cumsum([0] + [len(p[0]) for p in sets])
                pairs = np.concatenate([p[0] for p in sets])
                PT = torch.from_numpy(np.concatenate([p[1] for p in sets])).cuda()
                PL = None if sets[0][2] is None else torch.from_numpy(np.concatenate([p[2] for p in sets])).cuda()
                cons = lambda: ops.pose_graph_consistency(res.nodes, cat['edges'], dev['transforms'], dev['informations'], w, pairs=pairs,
                                                          pair_transforms=PT, pair_informations=PL, graph_node_offsets=noff,
                                                          graph_edge_offsets=eoff, graph_pair_offsets=poff)
                r = cons()  # warm-up
                torch.cuda.synchronize()
                ct = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = cons()
                    ct.append((time.perf_counter() - t0) * 1e3)
                assert torch.equal(r.covariances, m.covariances)
                d2 = r.d2[torch.isfinite(r.d2)]
                row['consistency_' + name] = {
                    'pairs': int(len(pairs)), 'columns': int(len(np.unique(pairs[:, 1] + np.repeat(noff[:-1], np.diff(poff))))),
                    'ms': float(np.median(ct)), 'ms_all': ct, 'per_marginals': float(np.median(ct)) / row['marginals_ms'],
                    'pair_status_1': int((r.pair_status != 0).sum()), 'd2_median': float(d2.median()) if len(d2) else None,
                    'd2_max': float(d2.max()) if len(d2) else None}
            row['_pairs_for_host'] = rand[0][0]
        return row

    out['one_graph'] = run(graphs[:1])
    out['batch_of_graphs'] = run(graphs)
    host_pairs = out['one_graph'].pop('_pairs_for_host', None)
    out['batch_of_graphs'].pop('_pairs_for_host', None)
    if a.cpu:
        c = graphs[0]
        t0 = time.perf_counter()
        res = R.optimize(c['nodes'], c['edges'], c['transforms'], c['informations'], c['uncertain'], MU, **TOL)
        out['host_dense'] = {'ms': (time.perf_counter() - t0) * 1e3, 'iterations': res['iterations'], 'cost': res['cost'],
                             'threads': os.environ.get('OMP_NUM_THREADS')}
        if a.marginals:
            H = R.normal_equations(res['nodes'], c['edges'], c['transforms'], c['informations'], c['uncertain'], MU)[0][6:, 6:]
            inv_ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                np.linalg.inv(H)
                inv_ms.append((time.perf_counter() - t0) * 1e3)
            out['host_dense_inverse'] = {'ms': float(np.median(inv_ms)), 'ms_all': inv_ms, 'unknowns': len(H),
                                         'threads': os.environ.get('OMP_NUM_THREADS')}
            if a.consistency:  # the dense route to the same pairs' blocks: the inverse, then 3 blocks per pair read out of it
                t0 = time.perf_counter()
                S = np.zeros((len(H) + 6, len(H) + 6))
                S[6:, 6:] = np.linalg.inv(H)
                blocks = [(S[6 * s:6 * s + 6, 6 * s:6 * s + 6], S[6 * t:6 * t + 6, 6 * t:6 * t + 6], S[6 * s:6 * s + 6, 6 * t:6 * t + 6])
                          for s, t in host_pairs.tolist()]
                out['host_dense_pair_blocks'] = {'ms': (time.perf_counter() - t0) * 1e3, 'pairs': len(blocks)}
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
