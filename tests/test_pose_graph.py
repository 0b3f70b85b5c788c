"""Pose-graph optimisation on the host: the restatement (tests/pose_graph_restatement.py) is checked against central differences
and solves the cases of tests/pose_graph_cases.py alone, so that the GPU tests may rely on it; the kernels' per-edge arithmetic,
compiled for the host (rdm_pose_graph_edge_terms_host, rdm_pose_graph_retract_host), equals the restatement's; the Python
wrapper's connectivity check."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_restatement as R

U = 2.0 ** -53


def test_analytic_jacobians_agree_with_central_differences():
    """Central difference with step h of a function with third derivative M3 and values known to eps: error <= h^2 M3 / 6 + eps / h.
    The residual's translation part is evaluated with eps ~ 16 2^-53 (|t_s| + |t_t| + |t_T|) <= 5e-13 on the 100 m poses, its third
    derivatives with respect to a rotation are below |u| <= 200: h = 1e-4 gives 200 * 1e-8 / 6 + 5e-13 / 1e-4 = 3.4e-7 + 5e-9; the
    bound is 1e-6.  Rotation parts: M3 < 1 for angles below 3, eps ~ 1e-15: 1.7e-9 + 1e-11."""
    h, bound = 1e-4, 1e-6
    rng = np.random.default_rng(0)
    worst = 0.0
    for k in range(40):
        Xs, Xt = cases.random_pose(rng), cases.random_pose(rng)
        angle = (1e-5, 1e-2, 0.3, 2.5)[k % 4]  # both sides of the series thresholds and a large residual
        T = R.retract(cases.inverse(Xt) @ Xs, cases.perturbation(rng, angle, 1.0))
        r, A, B = R.jacobians(Xs, Xt, T)
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            a = (R.residual(R.retract(Xs, d), Xt, T) - R.residual(R.retract(Xs, -d), Xt, T)) / (2 * h)
            b = (R.residual(Xs, R.retract(Xt, d), T) - R.residual(Xs, R.retract(Xt, -d), T)) / (2 * h)
            worst = max(worst, np.abs(a - A[:, j]).max(), np.abs(b - B[:, j]).max())
    print('largest difference', worst)
    assert worst <= bound


def test_series_and_closed_forms_meet_at_their_thresholds():
    rng = np.random.default_rng(1)
    for t2 in (R.SMALL_ANGLE2 * (1 - 1e-9), R.SMALL_ANGLE2 * (1 + 1e-9)):
        w = rng.normal(size=3)
        w *= np.sqrt(t2) / np.linalg.norm(w)
        assert np.abs(R.jr_inv(w) @ np.linalg.inv(R.jr_inv(w)) - np.eye(3)).max() < 1e-14
        back, _ = R.so3_log(R.so3_exp(w))
        assert np.abs(back - w).max() < 1e-15
    below, above = np.array([0.0, 0.0, np.sqrt(R.SMALL_ANGLE2)]) * (1 - 1e-9), np.array([0.0, 0.0, np.sqrt(R.SMALL_ANGLE2)]) * (1 + 1e-9)
    assert np.abs(R.jr_inv(below) - R.jr_inv(above)).max() < 1e-9 and np.abs(R.so3_exp(below) - R.so3_exp(above)).max() < 1e-9
    for s in (R.SMALL_SIN * 0.999, R.SMALL_SIN * 1.001):  # the rotation vector on both sides of its threshold
        w = np.array([s, 0.0, 0.0])
        back, _ = R.so3_log(R.so3_exp(w))
        assert np.abs(back - w).max() < 1e-18 + 4 * U * s


@pytest.mark.parametrize('name', cases.CONSISTENT)
def test_restatement_recovers_the_truth(name):
    """The options of the GPU test's solve except for the step count: the restatement's dense solve reaches the float64 floor
    within 8 steps on every case (a step of the 1 100-node case is a 6 594 x 6 594 dense solve: no more steps than needed)."""
    c = cases.consistent(name)
    res = R.optimize(c['nodes'], c['edges'], c['transforms'], c['informations'], max_iterations=8, gradient_tolerance=0.0,
                     cost_tolerance=0.0)
    ang, tra = R.pose_errors(res['nodes'], c['truth'])
    print(name, 'angle', ang, 'translation', tra, 'cost', res['cost0'], '->', res['cost'], res['iterations'])
    assert ang <= 1e-9 and tra <= 1e-9 and res['cost'] <= res['cost0']


def test_tree_has_no_cost_at_its_chained_poses():
    c = cases.tree()
    c['nodes'] = cases.chained_start(c)
    res = R.optimize(c['nodes'], c['edges'], c['transforms'], c['informations'])
    assert res['iterations'] == 0 and res['stop'] == R.STOP_GRADIENT and res['cost'] <= 1e-20
    assert R.pose_errors(c['nodes'], c['truth'])[1] > 0.05  # (the chained poses are not the truth: the edges are noisy)


def test_noisy_graph_every_loop_edge_matters():
    """The GPU test's cost bound (1e-10 relative) must break when one loop edge is dropped."""
    c = cases.noisy()
    full = R.optimize(c['nodes'], c['edges'], c['transforms'], c['informations'])
    assert full['stop'] in (R.STOP_GRADIENT, R.STOP_COST)
    for e in range(59, 69):
        keep = np.arange(69) != e
        less = R.optimize(c['nodes'], c['edges'][keep], c['transforms'][keep], c['informations'][keep])
        assert abs(less['cost'] - full['cost']) > 1e-2 * full['cost'], e
        # and the full graph's cost at the smaller graph's solution is far outside the bound
        assert R.cost(less['nodes'], c['edges'], c['transforms'], c['informations']) > (1 + 1e-6) * full['cost'], e


def test_line_process_separates_the_regimes():
    """mu = 1: with the gross loop edge (0.5 rad, 5 m) the restatement prunes exactly that edge and ends as near the truth as
    without the gross error; without a line process it ends several times further off."""
    mu = 1.0
    c, clean = cases.noisy(gross=3), cases.noisy()
    args = (c['edges'], c['transforms'], c['informations'], c['uncertain'])
    robust = R.optimize(c['nodes'], *args, mu)
    plain = R.optimize(c['nodes'], *args, None)
    base = R.optimize(clean['nodes'], clean['edges'], clean['transforms'], clean['informations'], clean['uncertain'], mu)
    assert np.nonzero(robust['weights'] < 0.25)[0].tolist() == [c['gross_edge']]
    assert robust['weights'][c['gross_edge']] < 1e-3 and np.delete(robust['weights'], c['gross_edge']).min() > 0.9
    assert base['weights'].min() > 0.9  # nothing is pruned from the clean graph
    noise, good, bad = (R.pose_errors(r['nodes'], c['truth']) for r in (base, robust, plain))
    print('noise', noise, 'line process', good, 'none', bad)
    assert good[0] < 1.2 * noise[0] and good[1] < 1.2 * noise[1]
    assert bad[0] > 3 * noise[0] and bad[1] > 3 * noise[1]


# ---- the kernels' arithmetic, compiled for the host ---------------------------------------------------------------------------

def test_native_edge_terms_equal_the_restatement():
    """rdm_pose_graph_edge_terms_host runs the functions the kernels run.  Per entry the two differ by rounding only: products of
    at most five 3 x 3 factors, a few hundred operations: 1e-11 relative to the largest entry of the block."""
    from rdmnet_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(2)
    for k in range(40):
        Xs, Xt = cases.random_pose(rng), cases.random_pose(rng)
        T = R.retract(cases.inverse(Xt) @ Xs, cases.perturbation(rng, (1e-5, 1e-2, 0.3, 2.5)[k % 4], 1.0))
        Lm = cases.random_information(rng)
        mu, unc = (3.0, 1) if k % 2 else (0.0, 0)
        out = np.zeros(128)
        assert L.rdm_pose_graph_edge_terms_host(Xs.ctypes.data, Xt.ctypes.data, T.ctypes.data, Lm.ctypes.data, mu, unc,
                                                out.ctypes.data) == 0
        r, A, B = R.jacobians(Xs, Xt, T)
        q = float(r @ Lm @ r)
        l = R.weight(q, mu if unc else None, bool(unc))
        want = [np.array([l]), np.array([R.edge_cost(q, l, mu if unc else None, bool(unc))]), r, l * A.T @ Lm @ A, l * A.T @ Lm @ B,
                l * B.T @ Lm @ B, l * A.T @ Lm @ r, l * B.T @ Lm @ r]
        at = 0
        for w in want:
            got = out[at:at + w.size].reshape(w.shape)
            at += w.size
            assert np.abs(got - w).max() <= 1e-11 * max(np.abs(w).max(), 1e-300), (k, at)
        assert at == 128
        d = cases.perturbation(rng, (1e-3, 0.09, 0.11, 2.0)[k % 4], 1.0)
        Y = np.zeros((4, 4))
        assert L.rdm_pose_graph_retract_host(Xs.ctypes.data, d.ctypes.data, Y.ctypes.data) == 0
        assert np.abs(Y - R.retract(Xs, d)).max() <= 1e-13 * 100


def test_native_edge_terms_refuse_an_angle_beyond_the_limit():
    from rdmnet_amd import _lib
    L = _lib.lib()
    X = np.eye(4)
    T = R.retract(np.eye(4), np.array([0.0, 0.0, 3.1, 0.0, 0.0, 0.0]))  # cos = -0.9991
    out = np.zeros(128)
    Lm = np.eye(6)
    assert L.rdm_pose_graph_edge_terms_host(X.ctypes.data, X.ctypes.data, T.ctypes.data, Lm.ctypes.data, 0.0, 0, out.ctypes.data) == -1
    with pytest.raises(ValueError):
        R.residual(X, X, T)
    T = R.retract(np.eye(4), np.array([0.0, 0.0, 2.9, 0.0, 0.0, 0.0]))
    assert L.rdm_pose_graph_edge_terms_host(X.ctypes.data, X.ctypes.data, T.ctypes.data, Lm.ctypes.data, 0.0, 0, out.ctypes.data) == 0
    assert np.abs(out[2:8] - R.residual(X, X, T)).max() < 1e-14


def test_wrapper_names_a_node_without_a_path_to_node_0():
    from rdmnet_amd import ops
    edges = np.array([[1, 0], [2, 1], [4, 3], [0, 1], [1, 2]])
    with pytest.raises(ValueError, match='node 3 of graph 0'):
        ops._pose_graph_connected(edges, np.array([0, 5, 8]), np.array([0, 3, 5]))
    ops._pose_graph_connected(edges[[0, 1, 3, 4]], np.array([0, 3, 6]), np.array([0, 2, 4]))
    with pytest.raises(ValueError, match='node 2 of graph 1'):
        ops._pose_graph_connected(edges[[0, 1, 3]], np.array([0, 3, 6]), np.array([0, 2, 3]))
    ops._pose_graph_connected(edges[:0], np.array([0, 3]), np.array([0, 0]))  # a graph without edges is returned as given
