"""GPU: ops.pose_graph_optimize(preconditioner='chain') -- the odometry-chain preconditioner of the conjugate gradients inside the
pose-graph solve -- against the float64 restatement and against the block-Jacobi path of the same build.

The preconditioner changes how fast the inner solve converges, never what it converges to: both paths end the inner solve at
sqrt(r^T M^-1 r) <= 1e-10 of its first value and the outer iteration by the same tolerances, so the bounds here are those of
tests/test_pose_graph_gpu.py (derived in its docstring): consistent graphs return to the truth within 1e-9, a noisy graph's final
cost is within 1e-10 relative of the restatement's."""
import numpy as np
import pytest
import torch

import pose_graph_cases as cases
import pose_graph_restatement as R
from rdmnet_amd import ops

pytestmark = pytest.mark.gpu

POSE_BOUND = 1e-9
REL_COST = 1e-10
TOLERANCES = dict(gradient_tolerance=1e-9, cost_tolerance=1e-12)
MU = 1.0
KEYS = ('nodes', 'edges', 'transforms', 'informations', 'uncertain')


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def solve(c, **kw):
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


# ---- 4. the same minimum ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['pair', 'ring3', 'ring40', 'double', 'hub', 'tree'])
def test_consistent_graphs_reach_the_truth(name):
    """The options of test_pose_graph_gpu.py's consistent solves: no tolerance ends them, 10 steps do.  tree() starts at the drive's
    true poses, 0.01 rad / 0.05 m per edge off what its noisy edges say; a tree's minimum is its chained poses (cost 0), and those
    are the truth it must reach."""
    c = cases.tree() if name == 'tree' else cases.consistent(name)
    if name == 'tree':
        c['truth'] = cases.chained_start(c)
    res = solve(c, max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0, preconditioner='chain')
    nodes = res.nodes.cpu().numpy()
    ang, tra = R.pose_errors(nodes, c['truth'])
    print(name, 'angle', ang, 'translation', tra, 'cost', res.initial_cost[0], '->', res.final_cost[0], 'iterations', res.iterations[0],
          'pcg', res.pcg_iterations[0], res.stop_reasons[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    assert res.final_cost[0] <= res.initial_cost[0]
    assert np.array_equal(nodes[0], c['nodes'][0])
    assert torch.equal(res.weights.cpu(), torch.ones(len(c['edges']), dtype=torch.float64)) and not res.pruned.any()


@pytest.mark.parametrize('gross', [None, 3])
def test_noisy_graphs_reach_the_restatement_s_cost(gross):
    """noisy() without a line process and noisy(gross=3) with mu = 1: the final cost, evaluated by the restatement, within REL_COST
    of R.optimize's; exactly the gross edge is pruned (nothing without one)."""
    c = cases.noisy(gross=gross)
    mu = MU if gross is not None else None
    res = solve(c, line_process_weight=mu, preconditioner='chain', **TOLERANCES)
    want = R.optimize(c['nodes'], *graph_args(c, mu), **TOLERANCES)
    got = R.cost(res.nodes.cpu().numpy(), *graph_args(c, mu))
    rel = (got - want['cost']) / want['cost']
    print('gross', gross, 'GPU cost', got, 'restatement', want['cost'], 'relative excess', rel, 'iterations', res.iterations[0],
          want['iterations'], res.stop_reasons[0], 'pcg', res.pcg_iterations[0])
    assert abs(rel) <= REL_COST
    assert res.stop_reason[0] in (1, 2)
    assert np.nonzero(res.pruned.cpu().numpy())[0].tolist() == ([c['gross_edge']] if gross is not None else [])


@pytest.mark.parametrize('which,gtol', [('noisy', 1e-8), ('ring40', 1e-7)])
def test_result_is_stationary(which, gtol):
    """Only the gradient test may end the solve: the restatement's gradient at the result is at most gradient_tolerance plus the
    evaluation's rounding (the cases and the allowance of tests/test_pose_graph_gpu.py)."""
    c = cases.noisy() if which == 'noisy' else cases.consistent(which)
    res = solve(c, gradient_tolerance=gtol, cost_tolerance=0.0, max_iterations=40, preconditioner='chain')
    assert res.stop_reason[0] == 1 and res.gradient_max[0] <= gtol
    nodes = res.nodes.cpu().numpy()
    g = np.abs(R.gradient(nodes, *graph_args(c))).max()
    rounding = gradient_rounding(c, nodes)
    print(which, 'gradient', g, 'tolerance', gtol, 'rounding allowance', rounding, 'iterations', res.iterations[0])
    assert g <= gtol + rounding


# ---- 5. a graph that is its chain -----------------------------------------------------------------------------------------------

def test_chain_only_graph_needs_one_pcg_iteration_per_step():
    """tree() from its first (truth-perturbed) start: M is the system, so conjugate gradients end after their first iteration; the
    factor 2 allows one more for rounding at the 1e-10 tolerance.  Block-Jacobi needs hundreds per step on the same call."""
    c = cases.tree()
    kw = dict(max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0)
    chain = solve(c, preconditioner='chain', **kw)
    plain = solve(c, preconditioner='block_jacobi', **kw)
    print('chain', chain.iterations[0], chain.pcg_iterations[0], 'block-Jacobi', plain.iterations[0], plain.pcg_iterations[0])
    assert chain.iterations[0] > 0 and chain.pcg_iterations[0] <= 2 * chain.iterations[0]
    assert plain.pcg_iterations[0] >= 100 * plain.iterations[0]
    minimum = cases.chained_start(c)
    for res in (chain, plain):
        ang, tra = R.pose_errors(res.nodes.cpu().numpy(), minimum)
        assert ang <= POSE_BOUND and tra <= POSE_BOUND


# ---- 6. a drive with loop closures ----------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize('mu', [None, MU])
def test_drive_with_loops_needs_a_quarter_of_the_iterations(mu):
    c = drive()
    kw = dict(line_process_weight=mu, max_iterations=30, **TOLERANCES)
    chain = solve(c, preconditioner='chain', **kw)
    plain = solve(c, preconditioner='block_jacobi', **kw)
    rel = abs(chain.final_cost[0] - plain.final_cost[0]) / plain.final_cost[0]
    print('mu', mu, 'chain: steps', chain.iterations[0], 'pcg', chain.pcg_iterations[0], chain.stop_reasons[0], 'block-Jacobi: steps',
          plain.iterations[0], 'pcg', plain.pcg_iterations[0], plain.stop_reasons[0], 'costs', chain.final_cost[0], plain.final_cost[0],
          'relative difference', rel)
    assert rel <= 1e-9
    assert chain.pcg_iterations[0] > 0 and 4 * chain.pcg_iterations[0] <= plain.pcg_iterations[0]


# ---- 7. direction and multiplicity ----------------------------------------------------------------------------------------------

def six_node_case():
    """Six nodes; the odometry edges alternate (i + 1, i) and (i, i + 1), the pair 2 - 3 carries two more edges, one in each direction,
    and one loop edge joins 5 and 1 (off the chain: diagonal only)."""
    rng = np.random.default_rng(12)
    edges = [(1, 0), (1, 2), (3, 2), (3, 4), (5, 4), (2, 3), (3, 2), (5, 1)]
    return cases.make([cases.random_pose(rng) for _ in range(6)], edges, rng)


@pytest.mark.parametrize('how', [dict(preconditioner='chain'), dict(linear_solver='direct')], ids=['chain', 'direct'])
def test_edge_direction_and_doubled_pairs(how):
    """six_node_case() under the chain preconditioner and under the direct solve, which add the same blocks by the same function."""
    c = six_node_case()
    res = solve(c, max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0, **how)
    ang, tra = R.pose_errors(res.nodes.cpu().numpy(), c['truth'])
    print('angle', ang, 'translation', tra, 'iterations', res.iterations[0], 'pcg', res.pcg_iterations[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    # without the loop edge M is the system, so (as on tree()) the conjugate gradients end after one iteration, two with rounding;
    # a block transposed the wrong way or a doubled edge left out would leave them the difference to work off
    keep = np.arange(len(c['edges'])) != 7
    d = dict(c, edges=c['edges'][keep], transforms=c['transforms'][keep], informations=c['informations'][keep], uncertain=c['uncertain'][keep])
    res = solve(d, max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0, **how)
    ang, tra = R.pose_errors(res.nodes.cpu().numpy(), c['truth'])
    print('without the loop edge: angle', ang, 'translation', tra, 'iterations', res.iterations[0], 'pcg', res.pcg_iterations[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    if 'preconditioner' in how:
        assert res.iterations[0] > 0 and res.pcg_iterations[0] <= 2 * res.iterations[0]
    else:
        assert res.iterations[0] > 0 and res.pcg_iterations[0] == 0


# ---- 8. batch invariance --------------------------------------------------------------------------------------------------------

def test_a_graph_is_the_same_alone_and_in_any_batch():
    a, b, d = cases.noisy(gross=3), cases.consistent('ring40'), cases.consistent('hub')
    kw = dict(line_process_weight=MU, preconditioner='chain', **TOLERANCES)

    def part(run, k):
        res, noff, eoff = run
        counters = [getattr(res, f)[k] for f in ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping',
                                                 'gradient_max')]
        return (res.nodes[noff[k]:noff[k + 1]], res.weights[eoff[k]:eoff[k + 1]], res.pruned[eoff[k]:eoff[k + 1]],
                torch.tensor(np.array(counters, np.float64)))

    alone, first, last = batch([a], **kw), batch([a, b, d], **kw), batch([d, b, a], **kw)
    for other in (part(first, 0), part(last, 2)):
        for x, y in zip(part(alone, 0), other):
            assert torch.equal(x.cpu(), y.cpu())
    assert part(alone, 0)[3][2] > 0 and part(alone, 0)[3][3] > 0  # (it iterated)


def test_a_batch_of_mixed_sizes_runs():
    """n = 1 (no free node), n = 2 (one free node: no off-diagonal block) and n = 60 in one call."""
    one = {k: cases.consistent('pair')[k][:1] if k == 'nodes' else cases.consistent('pair')[k][:0] for k in KEYS}
    two, sixty = cases.consistent('pair'), cases.noisy()
    res, noff, _ = batch([one, two, sixty], preconditioner='chain', **TOLERANCES)
    print(res.stop_reasons, res.iterations, res.pcg_iterations)
    assert res.stop_reasons[0] == 'empty' and res.iterations[0] == 0
    ang, tra = R.pose_errors(res.nodes[noff[1]:noff[2]].cpu().numpy(), two['truth'])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    alone = solve(sixty, preconditioner='chain', **TOLERANCES)
    assert torch.equal(alone.nodes, res.nodes[noff[2]:]) and alone.final_cost[0] == res.final_cost[2]


# ---- 9. the default is untouched ------------------------------------------------------------------------------------------------

def test_default_is_block_jacobi():
    c = cases.noisy()
    a = solve(c, **TOLERANCES)
    b = solve(c, preconditioner='block_jacobi', **TOLERANCES)
    for f in ('nodes', 'weights', 'pruned'):
        assert torch.equal(getattr(a, f), getattr(b, f))
    for f in ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping', 'gradient_max'):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    # and the chain is another computation with the same result
    d = solve(c, preconditioner='chain', **TOLERANCES)
    assert d.pcg_iterations[0] < a.pcg_iterations[0]
    assert abs(d.final_cost[0] - a.final_cost[0]) <= 1e-9 * a.final_cost[0]
