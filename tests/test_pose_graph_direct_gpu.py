"""GPU: ops.pose_graph_optimize(linear_solver='direct') -- the direct sparse solve in place of the conjugate gradients inside the
pose-graph optimisation -- against the float64 restatement and the chain-preconditioned path of the same
build.

The inner solver changes how the step of an outer iteration is computed, never what the iteration converges to, so the bounds are
those of tests/test_pose_graph_gpu.py (derived in its docstring) and tests/test_pose_graph_chain_gpu.py: consistent graphs return
to the truth within 1e-9 (rad and m) in ten steps, a noisy graph's final cost is within 1e-10 relative of the restatement's
optimum, two solvers' final costs agree to 1e-9 relative."""
import numpy as np
import pytest
import torch

import pose_graph_cases as cases
import pose_graph_restatement as R
from rdmnet_amd import _lib, ops

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-9
REL_COST = 1e-10
TOLERANCES = dict(gradient_tolerance=1e-9, cost_tolerance=1e-12)
TEN_STEPS = dict(max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0)
MU = 1.0
KEYS = ('nodes', 'edges', 'transforms', 'informations', 'uncertain')


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def solve(c, **kw):
    kw.setdefault('linear_solver', 'direct')
    return ops.pose_graph_optimize(dev(c['nodes']), c['edges'], dev(c['transforms']), dev(c['informations']), c['uncertain'], **kw)


def graph_args(c, mu=None):
    return c['edges'], c['transforms'], c['informations'], c['uncertain'], mu


def batch(graphs, **kw):
    noff = np.cumsum([0] + [len(g['nodes']) for g in graphs])
    eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
    cat = {k: np.concatenate([g[k] for g in graphs]) for k in KEYS}
    return solve(cat, graph_node_offsets=noff, graph_edge_offsets=eoff, **kw), noff, eoff


def gradient_rounding(c, nodes):
    """The rounding of the restatement's gradient evaluation (tests/test_pose_graph_gpu.py::test_result_is_stationary)."""
    u = 2.0 ** -53
    per_edge = 0.0
    for e, (s, t) in enumerate(c['edges']):
        r, A, B = R.jacobians(nodes[s], nodes[t], c['transforms'][e])
        scale = sum(np.linalg.norm(X[:3, 3]) for X in (nodes[s], nodes[t], c['transforms'][e]))
        dr = 16 * u * np.array([1.0, 1.0, 1.0, scale, scale, scale]) + 64 * u * np.abs(r)
        per_edge = max(per_edge, (2.0 * np.abs(np.concatenate([A, B], 1)).T @ np.abs(c['informations'][e]) @ dr).max())
    return np.bincount(c['edges'].reshape(-1)).max() * per_edge


# ---- 1. consistent graphs -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', cases.CONSISTENT)
def test_consistent_graphs_reach_the_truth(name):
    c = cases.consistent(name)
    res = solve(c, **TEN_STEPS)
    nodes = res.nodes.cpu().numpy()
    ang, tra = R.pose_errors(nodes, c['truth'])
    print(name, 'angle', ang, 'translation', tra, 'cost', res.initial_cost[0], '->', res.final_cost[0], 'iterations', res.iterations[0],
          'pcg', res.pcg_iterations[0], res.stop_reasons[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    assert res.pcg_iterations[0] == 0
    assert res.final_cost[0] <= res.initial_cost[0]
    assert np.array_equal(nodes[0], c['nodes'][0])
    assert torch.equal(res.weights.cpu(), torch.ones(len(c['edges']), dtype=torch.float64)) and not res.pruned.any()


# ---- 2. noisy graphs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('gross,mu', [(None, None), (None, MU), (3, MU)])
def test_noisy_graphs_reach_the_restatement_s_cost(gross, mu):
    c = cases.noisy(gross=gross)
    res = solve(c, line_process_weight=mu, **TOLERANCES)
    want = R.optimize(c['nodes'], *graph_args(c, mu), **TOLERANCES)
    got = R.cost(res.nodes.cpu().numpy(), *graph_args(c, mu))
    rel = (got - want['cost']) / want['cost']
    print('gross', gross, 'mu', mu, 'GPU cost', got, 'restatement', want['cost'], 'relative excess', rel, 'iterations', res.iterations[0],
          want['iterations'], res.stop_reasons[0])
    assert abs(rel) <= REL_COST
    assert res.stop_reason[0] in (1, 2) and res.pcg_iterations[0] == 0
    assert np.nonzero(res.pruned.cpu().numpy())[0].tolist() == ([c['gross_edge']] if gross is not None else [])


def test_result_is_stationary():
    """Only the gradient test may end the solve: the restatement's gradient at the result is at most gradient_tolerance plus the
    evaluation's rounding (the case and the allowance of tests/test_pose_graph_gpu.py)."""
    c, gtol = cases.noisy(), 1e-8
    res = solve(c, gradient_tolerance=gtol, cost_tolerance=0.0, max_iterations=40)
    assert res.stop_reason[0] == 1 and res.gradient_max[0] <= gtol
    nodes = res.nodes.cpu().numpy()
    g = np.abs(R.gradient(nodes, *graph_args(c))).max()
    rounding = gradient_rounding(c, nodes)
    print('gradient', g, 'tolerance', gtol, 'rounding allowance', rounding, 'iterations', res.iterations[0])
    assert g <= gtol + rounding


# ---- 3. the same minimum as the chain-preconditioned conjugate gradients ------------------------------------------------------

def drive(n=150, loops=8, seed=40):
    """tools/pose_graph_bench.graph at 150 scans: loops from a node s >= 80 back by 20 .. 80."""
    rng = np.random.default_rng(seed)
    truth = cases.trajectory_truth(rng, n)
    odo = [(i + 1, i) for i in range(n - 1)]
    loop = [(int(s), int(s) - int(rng.integers(20, 80))) for s in rng.choice(np.arange(80, n), size=loops, replace=False)]
    c = cases.make(truth, odo + loop, rng, start_angle=0.0, start_distance=0.0, noise_angle=0.01, noise_distance=0.05,
                   uncertain=[0] * len(odo) + [1] * len(loop))
    c['nodes'] = cases.chained_start(c)
    return c


@pytest.mark.parametrize('which,mu', [('noisy', None), ('drive', None), ('drive', MU)])
def test_direct_and_chain_end_at_the_same_cost(which, mu):
    c = cases.noisy() if which == 'noisy' else drive()
    kw = dict(line_process_weight=mu, max_iterations=30, **TOLERANCES)
    direct = solve(c, **kw)
    chain = solve(c, linear_solver='pcg', preconditioner='chain', **kw)
    rel = abs(direct.final_cost[0] - chain.final_cost[0]) / chain.final_cost[0]
    print(which, 'mu', mu, 'direct: steps', direct.iterations[0], direct.stop_reasons[0], 'chain: steps', chain.iterations[0], 'pcg',
          chain.pcg_iterations[0], chain.stop_reasons[0], 'costs', direct.final_cost[0], chain.final_cost[0], 'relative difference', rel)
    assert rel <= 1e-9
    assert direct.pcg_iterations[0] == 0 and chain.pcg_iterations[0] > 0


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------

def test_a_graph_is_the_same_alone_and_in_any_batch():
    a, pair, ring3, ring40 = cases.noisy(), cases.consistent('pair'), cases.consistent('ring3'), cases.consistent('ring40')
    kw = dict(line_process_weight=MU, **TOLERANCES)

    def part(run, k):
        res, noff, eoff = run
        counters = [getattr(res, f)[k] for f in ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping',
                                                 'gradient_max')]
        return (res.nodes[noff[k]:noff[k + 1]], res.weights[eoff[k]:eoff[k + 1]], res.pruned[eoff[k]:eoff[k + 1]],
                torch.tensor(np.array(counters, np.float64)))

    alone, again = batch([a], **kw), batch([a], **kw)
    last, first = batch([pair, ring3, a], **kw), batch([a, ring40, pair], **kw)
    for other in (part(again, 0), part(last, 2), part(first, 0)):
        for x, y in zip(part(alone, 0), other):
            assert torch.equal(x.cpu(), y.cpu())
    assert part(alone, 0)[3][2] > 0  # (it iterated)


# ---- 5. the small shapes ----------------------------------------------------------------------------------------------------

SHAPES = {
    'separator at node 1': (5, [(1, 3)]),
    'separator at the last node': (8, [(7, 2), (7, 4)]),
    'adjacent separators': (14, [(3, 6), (3, 8), (4, 10), (4, 12)]),
    'chord between separators': (14, [(3, 6), (3, 8), (10, 5), (10, 12), (3, 10)]),
    'double edge between separators': (14, [(3, 6), (3, 8), (10, 5), (10, 12), (3, 10), (3, 10)]),
    'run of one node': (12, [(3, 7), (3, 9), (5, 1), (5, 11)]),
    'chain of 300 with one chord': (300, [(10, 290)]),
}


@pytest.mark.parametrize('name', list(SHAPES))
def test_small_shapes_reach_the_truth(name):
    n, chords = SHAPES[name]
    rng = np.random.default_rng(300 + n + len(chords))
    c = cases.make([cases.random_pose(rng) for _ in range(n)], [(i + 1, i) for i in range(n - 1)] + chords, rng)
    res = solve(c, **TEN_STEPS)
    ang, tra = R.pose_errors(res.nodes.cpu().numpy(), c['truth'])
    print(name, 'angle', ang, 'translation', tra, 'cost', res.initial_cost[0], '->', res.final_cost[0], 'iterations', res.iterations[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    assert res.pcg_iterations[0] == 0


# ---- 6. graphs without work, and the cap --------------------------------------------------------------------------------------

def test_graphs_without_nodes_or_edges_are_returned_as_given():
    pair = cases.consistent('pair')
    ring3 = cases.consistent('ring3')
    empty = {k: pair[k][:0] for k in KEYS}
    one = {k: pair[k][:1] if k == 'nodes' else pair[k][:0] for k in KEYS}
    no_edges = {k: ring3[k] if k == 'nodes' else ring3[k][:0] for k in KEYS}
    res, noff, _ = batch([empty, one, no_edges, pair], **TOLERANCES)
    print(res.stop_reasons, res.iterations)
    assert res.stop_reasons[:3] == ['empty'] * 3 and res.iterations[:3].tolist() == [0, 0, 0]
    assert np.array_equal(res.nodes[noff[1]:noff[2]].cpu().numpy(), one['nodes'])
    assert np.array_equal(res.nodes[noff[2]:noff[3]].cpu().numpy(), no_edges['nodes'])
    ang, tra = R.pose_errors(res.nodes[noff[3]:].cpu().numpy(), pair['truth'])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND


def test_a_graph_over_the_cap_is_refused_and_nothing_is_written():
    L = _lib.lib()
    k = L.rdm_pose_graph_direct_max_separator() + 1
    n = 3 * k + 4
    edges = np.array([(i + 1, i) for i in range(n - 1)] + [(3 * j + 1, 3 * j + 3) for j in range(k)], np.int64)
    e = len(edges)
    X = torch.eye(4, dtype=torch.float64, device='cuda').repeat(n, 1, 1).contiguous()
    T = torch.eye(4, dtype=torch.float64, device='cuda').repeat(e, 1, 1).contiguous()
    Lm = torch.eye(6, dtype=torch.float64, device='cuda').repeat(e, 1, 1).contiguous()
    with pytest.raises(RuntimeError, match=str(k)):
        ops.pose_graph_optimize(X, edges, T, Lm, linear_solver='direct')
    # the library itself: RDM_ERR_ARG, and every output keeps what it held
    out = torch.full_like(X, -3.0)
    weights = torch.full((e,), -3.0, dtype=torch.float64, device='cuda')
    pruned = torch.full((e,), 9, dtype=torch.uint8, device='cuda')
    report = np.full((1, 8), -3.0)
    noff, eoff = np.array([0, n], np.int64), np.array([0, e], np.int64)
    ws = torch.empty(L.rdm_pose_graph_workspace_bytes_pc(1, n, e, 1), dtype=torch.uint8, device='cuda')
    rc = L.rdm_pose_graph_optimize_ls(1, noff.ctypes.data, eoff.ctypes.data, X.data_ptr(), edges.ctypes.data, T.data_ptr(), Lm.data_ptr(), 0,
                                      0.0, 0.25, 10, 1e-9, 1e-12, 100, 1e-10, 0, 1, out.data_ptr(), weights.data_ptr(), pruned.data_ptr(),
                                      report.ctypes.data, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = L.rdm_last_error().decode()
    print(rc, msg)
    assert rc == -1 and str(k) in msg and str(k - 1) in msg
    assert bool((out == -3.0).all()) and bool((weights == -3.0).all()) and bool((pruned == 9).all()) and np.all(report == -3.0)
    # linear_solver 2 does not exist
    rc = L.rdm_pose_graph_optimize_ls(1, noff.ctypes.data, eoff.ctypes.data, X.data_ptr(), edges.ctypes.data, T.data_ptr(), Lm.data_ptr(), 0,
                                      0.0, 0.25, 10, 1e-9, 1e-12, 100, 1e-10, 0, 2, out.data_ptr(), weights.data_ptr(), pruned.data_ptr(),
                                      report.ctypes.data, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    assert rc == -1 and bool((out == -3.0).all())


# ---- 7. the default is untouched ----------------------------------------------------------------------------------------------

def test_default_is_the_conjugate_gradients():
    c = cases.noisy()
    a = ops.pose_graph_optimize(dev(c['nodes']), c['edges'], dev(c['transforms']), dev(c['informations']), c['uncertain'], **TOLERANCES)
    b = solve(c, linear_solver='pcg', **TOLERANCES)
    for f in ('nodes', 'weights', 'pruned'):
        assert torch.equal(getattr(a, f), getattr(b, f))
    for f in ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping', 'gradient_max'):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    assert a.pcg_iterations[0] > 0
