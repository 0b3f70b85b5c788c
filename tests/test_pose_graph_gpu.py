"""GPU: rdm_pose_graph_optimize through ops.pose_graph_optimize and `python -m rdmnet_amd.trajectory --optimize`, against the
float64 restatement (tests/pose_graph_restatement.py) on the graphs of tests/pose_graph_cases.py (tests/test_pose_graph.py shows
on the host that the restatement alone solves them).

The cost bound of the noisy graph and of the line process (REL_COST = 1e-10).  Both solvers are run with
cost_tolerance = 1e-12 and gradient_tolerance = 1e-9 and end by one of the two tests.  A solve that ends by the cost test took a
last step that lowered F by at most 1e-12 F; Gauss-Newton on these small-residual graphs contracts by a factor rho well below
0.99 per step near the minimum, so what is left to the minimum is at most rho / (1 - rho) < 100 such decreases, 1e-10 F.  A solve
that ends by the gradient test is within g^T H^-1 g / 4 of the minimum, which for |g| <= 1e-9 and the blocks of these graphs
(smallest eigenvalue of H above 1e-3) is below 1e-12.  So each final cost lies within 1e-10 F of the minimum's and they lie within
1e-10 F of each other; the evaluation itself (fsum of 69 terms of ~20 rounded operations) adds 1e-14.  Measured on an MI355X:
the noisy graph's relative difference is 1.8e-13 (12 iterations against the restatement's 13, both ended by the cost test), the
line process's 8.9e-16 (21 iterations each).
Dropping one loop edge of the noisy graph changes its minimal cost by more than 1e-2 of it (test_pose_graph.py asserts this
for every loop edge)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pose_graph_cases as cases
import pose_graph_restatement as R
from rdmnet_amd import ops

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
POSE_BOUND = 1e-9        # the project's bound for float64 results
REL_COST = 1e-10         # allowed relative excess of the GPU's final cost over the restatement's (derived above)
TOLERANCES = dict(gradient_tolerance=1e-9, cost_tolerance=1e-12)
MU = 1.0                 # the line process weight of test 5 (test_pose_graph.py: the restatement separates the regimes with it)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def solve(c, **kw):
    return ops.pose_graph_optimize(dev(c['nodes']), c['edges'], dev(c['transforms']), dev(c['informations']), c['uncertain'], **kw)


def graph_args(c, mu=None):
    return c['edges'], c['transforms'], c['informations'], c['uncertain'], mu


_cache = {}


def consistent_result(name):
    """One solve per consistent case, shared by the tests (float64 floor: no tolerance ends it, 10 steps do; the restatement needs 7)."""
    if name not in _cache:
        c = cases.consistent(name)
        _cache[name] = (c, solve(c, max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0))
    return _cache[name]


def noisy_result():
    if 'noisy' not in _cache:
        c = cases.noisy()
        _cache['noisy'] = (c, solve(c, **TOLERANCES), R.optimize(c['nodes'], *graph_args(c), **TOLERANCES))
    return _cache['noisy']


@pytest.mark.parametrize('name', cases.CONSISTENT)
def test_consistent_graphs_reach_the_truth(name):
    c, res = consistent_result(name)
    nodes = res.nodes.cpu().numpy()
    ang, tra = R.pose_errors(nodes, c['truth'])
    print(name, 'angle', ang, 'translation', tra, 'cost', res.initial_cost[0], '->', res.final_cost[0], 'iterations', res.iterations[0],
          'pcg', res.pcg_iterations[0], res.stop_reasons[0])
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    assert res.final_cost[0] <= res.initial_cost[0]
    assert np.array_equal(nodes[0], c['nodes'][0])  # node 0 is fixed
    assert torch.equal(res.weights.cpu(), torch.ones(len(c['edges']), dtype=torch.float64)) and not res.pruned.any()


def test_tree_keeps_its_chained_poses():
    c = cases.tree()
    c['nodes'] = cases.chained_start(c)
    res = solve(c)
    nodes = res.nodes.cpu().numpy()
    print('tree cost', res.initial_cost[0], res.final_cost[0], 'iterations', res.iterations[0], res.stop_reasons[0],
          'largest change', np.abs(nodes - c['nodes']).max())
    assert np.abs(nodes - c['nodes']).max() <= 1e-12
    assert 0.0 <= res.final_cost[0] <= 1e-20  # 49 edges, residuals of a few 1e-15 on this 100 m drive, information entries ~10


def test_noisy_graph_cost_equals_the_restatement():
    """The GPU's final cost, evaluated by the restatement, against the restatement's own: REL_COST (module docstring); measured on an
    MI355X: 1.8e-13."""
    c, res, want = noisy_result()
    got = R.cost(res.nodes.cpu().numpy(), *graph_args(c))
    rel = (got - want['cost']) / want['cost']
    print('noisy: GPU cost', got, 'as reported', res.final_cost[0], 'restatement', want['cost'], 'relative excess', rel, 'iterations',
          res.iterations[0], want['iterations'], res.stop_reasons[0], 'pcg', res.pcg_iterations[0])
    assert abs(rel) <= REL_COST
    assert abs(res.final_cost[0] - got) <= 1e-12 * got  # the device's own sum of the same terms
    assert res.stop_reason[0] in (1, 2) and want['stop'] in (1, 2)


@pytest.mark.parametrize('which,gtol', [('noisy', 1e-8), ('ring40', 1e-7)])
def test_result_is_stationary(which, gtol):
    """A solve that only the gradient test may end (cost_tolerance = 0): the restatement's gradient at the GPU's result is at most
    the call's gradient_tolerance plus the evaluation's rounding.  The rounding: a residual carries an absolute error of about
    16 2^-53 (rotation) and 16 2^-53 (|t_s| + |t_t| + |t_T|) (translation: the positions cancel) and 64 2^-53 of itself; an edge
    passes it on through 2 |J|^T |L|, and a node adds its edges.  On the noisy graph a solver with approximate Jacobians (the
    rotation block without the inverse right Jacobian) stops at a point whose true gradient is larger by orders of magnitude.
    The consistent 40-ring cannot tell: its residuals vanish at the solution, so J^T L r tends to 0 for any J; it holds the
    gradient test and the report's gradient_max on a 100 m scale.  The Jacobians themselves are also held entry by entry on
    the host (test_pose_graph.py::test_native_edge_terms_equal_the_restatement)."""
    c = cases.noisy() if which == 'noisy' else cases.consistent(which)
    res = solve(c, gradient_tolerance=gtol, cost_tolerance=0.0, max_iterations=40)
    assert res.stop_reason[0] == 1 and res.gradient_max[0] <= gtol
    nodes = res.nodes.cpu().numpy()
    g = np.abs(R.gradient(nodes, *graph_args(c))).max()
    u = 2.0 ** -53
    per_edge = 0.0
    for e, (s, t) in enumerate(c['edges']):
        r, A, B = R.jacobians(nodes[s], nodes[t], c['transforms'][e])
        scale = sum(np.linalg.norm(X[:3, 3]) for X in (nodes[s], nodes[t], c['transforms'][e]))
        dr = 16 * u * np.array([1.0, 1.0, 1.0, scale, scale, scale]) + 64 * u * np.abs(r)
        per_edge = max(per_edge, (2.0 * np.abs(np.concatenate([A, B], 1)).T @ np.abs(c['informations'][e]) @ dr).max())
    degree = np.bincount(c['edges'].reshape(-1)).max()
    rounding = degree * per_edge
    print(which, 'gradient', g, 'tolerance', gtol, 'rounding allowance', rounding, 'gpu gradient', res.gradient_max[0], 'iterations',
          res.iterations[0])
    assert g <= gtol + rounding


def test_line_process_prunes_the_gross_edge():
    c = cases.noisy(gross=3)
    res = solve(c, line_process_weight=MU, **TOLERANCES)
    want = R.optimize(c['nodes'], *graph_args(c, MU), **TOLERANCES)
    pruned = res.pruned.cpu().numpy()
    weights = res.weights.cpu().numpy()
    got = R.cost(res.nodes.cpu().numpy(), *graph_args(c, MU))
    rel = (got - want['cost']) / want['cost']
    ang, tra = R.pose_errors(res.nodes.cpu().numpy(), want['nodes'])
    print('line process: pruned', np.nonzero(pruned)[0], 'gross edge', c['gross_edge'], 'weights', weights[59:], 'relative cost excess',
          rel, 'pose difference to the restatement', ang, tra, 'iterations', res.iterations[0], want['iterations'])
    assert np.nonzero(pruned)[0].tolist() == [c['gross_edge']]
    assert abs(rel) <= REL_COST
    # poses: the two run the same iteration (start, damping schedule, accept rule) and differ in the linear solve alone, conjugate
    # gradients to 1e-10 of the first residual against LU: a step differs by about 1e-10 of its length, the 21 steps add up to a
    # few metres, and near the minimum the iteration contracts, so the differences do not grow: POSE_BOUND, the project's bound for
    # float64 results (measured: 4.5e-14 rad, 4.8e-13 m).  Weights: |dl / dq| <= 2 / mu and dq = 2 r^T L J dx with |L r| < 1,
    # |J| < 50 (the lever arms of this drive) and |dx| <= 1e-9: 1e-7.
    assert ang <= POSE_BOUND and tra <= POSE_BOUND
    assert np.all(weights[:59] == 1.0) and np.allclose(weights, want['weights'], rtol=0, atol=1e-7)
    plain = solve(c, **TOLERANCES)
    assert not plain.pruned.any() and torch.equal(plain.weights.cpu(), torch.ones(69, dtype=torch.float64))
    off = R.optimize(c['nodes'], *graph_args(c), **TOLERANCES)
    clean = cases.noisy()
    noise = R.pose_errors(R.optimize(clean['nodes'], *graph_args(clean), **TOLERANCES)['nodes'], clean['truth'])
    spoiled = R.pose_errors(off['nodes'], c['truth'])
    print('without the line process: off the truth by', spoiled, 'noise alone', noise)
    assert spoiled[0] > 3 * noise[0] and spoiled[1] > 3 * noise[1]


def test_a_graph_is_the_same_alone_and_in_any_batch():
    a, b, d = cases.noisy(gross=3), cases.consistent('ring40'), cases.consistent('hub')

    def batch(graphs):
        noff = np.cumsum([0] + [len(g['nodes']) for g in graphs])
        eoff = np.cumsum([0] + [len(g['edges']) for g in graphs])
        cat = {k: np.concatenate([g[k] for g in graphs]) for k in ('nodes', 'edges', 'transforms', 'informations', 'uncertain')}
        res = solve(cat, line_process_weight=MU, graph_node_offsets=noff, graph_edge_offsets=eoff, **TOLERANCES)
        return res, noff, eoff

    def part(run, k):
        res, noff, eoff = run
        counters = [getattr(res, f)[k] for f in ('initial_cost', 'final_cost', 'iterations', 'pcg_iterations', 'stop_reason', 'damping',
                                                 'gradient_max')]
        return (res.nodes[noff[k]:noff[k + 1]].cpu().numpy(), res.weights[eoff[k]:eoff[k + 1]].cpu().numpy(),
                res.pruned[eoff[k]:eoff[k + 1]].cpu().numpy(), np.array(counters, np.float64))

    alone, first, last, again = batch([a]), batch([a, b, d]), batch([d, b, a]), batch([d, b, a])
    for other in (part(first, 0), part(last, 2), part(again, 2)):
        for x, y in zip(part(alone, 0), other):
            assert np.array_equal(x, y)
    for k in range(3):
        for x, y in zip(part(last, k), part(again, k)):
            assert np.array_equal(x, y)
    assert part(alone, 0)[3][2] > 0  # (it iterated)


def test_argument_errors_leave_the_outputs_untouched():
    c = cases.consistent('ring3')

    def attempt(exc, match, **change):
        d = dict(c, **change)
        X = dev(d['nodes'])
        before = X.clone()
        with pytest.raises(exc, match=match):
            ops.pose_graph_optimize(X, d['edges'], dev(d['transforms']), dev(d['informations']), d['uncertain'], **d.get('kw', {}))
        assert torch.equal(X.view(torch.int64), before.view(torch.int64))  # (the inputs; the C outputs: the next test)

    edges = c['edges'].copy()
    edges[1] = (2, 2)
    attempt(RuntimeError, 'itself', edges=edges)
    edges = c['edges'].copy()
    edges[1] = (2, 3)
    attempt(RuntimeError, 'outside graph', edges=edges)
    nodes = c['nodes'].copy()
    nodes[1, 0, 3] = np.nan
    attempt(RuntimeError, 'not finite', nodes=nodes)
    infos = c['informations'].copy()
    infos[2, 1, 4] += 1e-3
    attempt(RuntimeError, 'not symmetric', informations=infos)
    # a node that no path connects to node 0: 4 nodes, node 3 joined to nobody; and 5 nodes with 3 - 4 joined to each other only
    four = np.concatenate([c['nodes'], c['nodes'][:1]])
    attempt(ValueError, 'node 3 of graph 0', nodes=four)
    five = np.concatenate([c['nodes'], c['nodes'][:2]])
    attempt(ValueError, 'node 3 of graph 0', nodes=five, edges=np.concatenate([c['edges'], [[3, 4]]]),
            transforms=np.concatenate([c['transforms'], c['transforms'][:1]]),
            informations=np.concatenate([c['informations'], c['informations'][:1]]), uncertain=np.zeros(4, np.uint8))
    # over the limits: 65 537 nodes in a chain
    n = ops.POSE_GRAPH_MAX_NODES + 1
    chain = np.stack([np.arange(1, n), np.arange(0, n - 1)], 1)
    eye = np.broadcast_to(np.eye(4), (n, 4, 4))
    attempt(RuntimeError, 'limits', nodes=np.ascontiguousarray(eye), edges=chain, transforms=np.ascontiguousarray(eye[1:]),
            informations=np.ascontiguousarray(np.broadcast_to(np.eye(6), (n - 1, 6, 6))), uncertain=np.zeros(n - 1, np.uint8))


def test_failed_calls_leave_the_c_outputs_untouched():
    """rdm_pose_graph_optimize itself, with nodes_out = nodes in place and sentinel weights / flags, on a batch of a sound graph and a
    faulty one: the two causes the input check finds (a NaN pose, an asymmetric information matrix) and the two found during the
    solve (a residual rotation of the given poses beyond the angle limit, a node block that is not positive definite).  Every
    output stays as it was, the message names graph 1 and its cause, the report carries the status."""
    from rdmnet_amd import _lib
    L = _lib.lib()
    c = cases.consistent('ring3')
    nan = c['nodes'].copy()
    nan[1, 0, 3] = np.nan
    asym = c['informations'].copy()
    asym[2, 1, 4] += 1e-3
    turned = c['nodes'].copy()
    turned[1] = R.retract(c['truth'][1], np.array([0.0, 0.0, 3.1, 0.0, 0.0, 0.0]))  # cos of the residual angle = -0.9991
    faults = [(1, 'not finite', dict(nodes=nan)), (2, 'not symmetric', dict(informations=asym)),
              (3, 'beyond the supported angle', dict(nodes=turned)),
              (4, 'not positive definite', dict(informations=np.zeros_like(c['informations'])))]
    off = np.array([0, 3, 6], np.int64)
    edges = np.ascontiguousarray(np.concatenate([c['edges'], c['edges']]))
    for status, text, change in faults:
        d = dict(c, **change)
        given = np.concatenate([c['nodes'], d['nodes']])
        X, T = dev(given), dev(np.concatenate([c['transforms'], d['transforms']]))
        Lm = dev(np.concatenate([c['informations'], d['informations']]))
        sentinel = torch.full((6,), -7.0, dtype=torch.float64, device='cuda')
        flags = torch.full((6,), 9, dtype=torch.uint8, device='cuda')
        report = np.zeros((2, 8))
        ws = ops.scratch(X.device, L.rdm_pose_graph_workspace_bytes(2, 6, 6))
        rc = L.rdm_pose_graph_optimize(2, off.ctypes.data, off.ctypes.data, X.data_ptr(), edges.ctypes.data, T.data_ptr(), Lm.data_ptr(),
                                       0, 0.0, 0.25, 10, 1e-9, 1e-12, 100, 1e-10, X.data_ptr(), sentinel.data_ptr(), flags.data_ptr(),
                                       report.ctypes.data, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        message = L.rdm_last_error().decode()
        print(status, rc, message, report[:, 5])
        assert rc == -1 and 'graph 1' in message and text in message
        assert report[0, 5] == 0 and report[1, 5] == status
        assert torch.equal(X.view(torch.int64), dev(given).view(torch.int64))  # (bit patterns: a NaN stays the NaN it was)
        assert (sentinel == -7.0).all() and (flags == 9).all()


def test_empty_graphs_return_at_once():
    c = cases.consistent('ring3')
    res = ops.pose_graph_optimize(dev(c['nodes']), np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    assert np.array_equal(res.nodes.cpu().numpy(), c['nodes']) and res.final_cost[0] == 0.0 and res.iterations[0] == 0
    assert res.stop_reasons == ['empty'] and res.weights.numel() == 0
    res = ops.pose_graph_optimize(np.zeros((0, 4, 4)), np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), np.zeros((0, 6, 6)))
    assert res.nodes.shape == (0, 4, 4) and res.final_cost[0] == 0.0 and res.iterations[0] == 0
    # an empty graph between two others of a batch
    noff, eoff = np.array([0, 3, 3, 6]), np.array([0, 3, 3, 6])
    two = {k: np.concatenate([c[k], c[k]]) for k in ('nodes', 'edges', 'transforms', 'informations', 'uncertain')}
    res = solve(two, graph_node_offsets=noff, graph_edge_offsets=eoff, max_iterations=10, gradient_tolerance=0.0, cost_tolerance=0.0)
    assert res.stop_reasons[1] == 'empty' and res.iterations[1] == 0 and res.iterations[0] == res.iterations[2] > 0
    assert torch.equal(res.nodes[:3], res.nodes[3:])


def test_cli_optimizes_two_sequences(tmp_path):
    """`python -m rdmnet_amd.trajectory --optimize` as a fresh child process on synthetic pair files of two sequences with
    information matrices and one loop edge each."""
    root, out = tmp_path / 'pairs', tmp_path / 'traj'
    root.mkdir()
    for seq, seed, n in ((9, 21, 12), (10, 22, 8)):
        rng = np.random.default_rng(seed)
        truth = cases.trajectory_truth(rng, n)
        frames = [10 * i for i in range(n)]
        pairs = [(i, i + 1) for i in range(n - 1)] + [(n - 1, 0)]  # (src node, ref node); the last is the loop
        for s, t in pairs:
            gt = cases.inverse(truth[t]) @ truth[s]
            est = R.retract(gt, cases.perturbation(rng, 0.01, 0.05))
            np.savez(str(root / f'{seq}_{frames[s]}_{frames[t]}.npz'), estimated_transform=est, transform=gt,
                     information=cases.random_information(rng))
    p = subprocess.run([sys.executable, '-m', 'rdmnet_amd.trajectory', '--features-root', str(root), '--optimize',
                        '--line-process-weight', '5', '--out', str(out)], cwd=REPO, capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0
    lines = p.stdout.strip().splitlines()
    for seq, n in ((9, 12), (10, 8)):
        assert sum(l.startswith(f'seq {seq} chained: r_rmse: ') for l in lines) == 1
        assert sum(l.startswith(f'seq {seq} optimized: r_rmse: ') for l in lines) == 1
        graph = [l for l in lines if l.startswith(f'seq {seq} pose graph: {n} nodes, {n} edges, cost ')]
        assert len(graph) == 1 and 'iterations' in graph[0] and graph[0].endswith('pruned edges: []')
        before, after = (float(v) for v in graph[0].split('cost ')[1].split(',')[0].split(' -> '))
        assert after < before
        for variant in ('chained', 'optimized'):
            assert np.loadtxt(str(out / f'{seq}_{variant}.txt')).shape == (n, 12)  # one pose per frame
