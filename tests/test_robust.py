"""CPU: the float64 restatement of the robust estimator (tests/robust_restatement.py) on its own fixtures, the tie rule of the
maximum clique, and the host side of `python -m rdmnet_amd.eval --method robust`.

Pose bounds of the planted fixtures.  The planted rows carry noise of norm <= 0.45 noise_bound each.  The translation estimate of
an axis is a mean over rows that all lie within noise_bound of it, so it is off by less than noise_bound plus the rotation error
times the lever arm (<= 70 m); the rotation comes from >= 190 measurement pairs with baselines of tens of metres and noise
<= 0.9 noise_bound each, which keeps it below 0.9 noise_bound / 10 m = 4.5e-3 rad even for a single 10 m pair; asserted:
0.02 degrees (3.5e-4 rad) and one noise_bound."""
import numpy as np
import pytest

import robust_restatement as RR
from rdmnet_amd import _lib
from rdmnet_amd import eval as cli

PLANTED = [(65, 20, 0.01), (129, 40, 0.01), (300, 120, 0.01), (300, 60, 0.05)]


@pytest.mark.parametrize('C,n_in,beta', PLANTED)
def test_restatement_recovers_the_planted_rows_and_pose(C, n_in, beta):
    src, ref, rows, poses = RR.make_fixture(C, n_in, beta, seed=C + n_in)
    res = RR.robust_registration(src, ref, beta)
    RR.check_fixture(res)
    assert np.array_equal(res.selected, rows[0]) and res.valid == 1 and res.translation_inliers == n_in
    assert res.threshold_margin >= 2e-4
    rre, rte = RR.pose_error(res.transform, poses[0])
    print(C, n_in, beta, 'rre', rre, 'rte', rte, 'margins', res.threshold_margin, res.cost_margin)
    assert rre < 0.02 and rte < beta
    assert np.array_equal(res.transform[3], [0, 0, 0, 1])
    assert np.array_equal(res.degree, res.adjacency.sum(1)) and res.core[rows[0]].min() >= n_in - 1


def test_two_equal_groups_the_lower_first_row_wins():
    src, ref, rows, poses = RR.make_fixture(129, 30, 0.01, seed=11, groups=2)
    res = RR.robust_registration(src, ref, 0.01)
    RR.check_fixture(res, unique_clique=False)
    cliques = RR.maximum_cliques(res.adjacency)
    assert sorted(cliques) == sorted(tuple(r) for r in rows)  # exactly the two planted groups
    first = min(rows, key=lambda r: r[0])
    assert np.array_equal(res.selected, first)
    which = 0 if first is rows[0] else 1
    rre, rte = RR.pose_error(res.transform, poses[which])
    assert rre < 0.02 and rte < 0.01
    # the rule itself, on a hand-made graph: {0, 3, 4} and {1, 2, 5} and {0, 2, 5} are all maximum; (0, 2, 5) < (0, 3, 4) < (1, 2, 5)
    adj = np.zeros((6, 6), bool)
    for c in ((0, 3, 4), (1, 2, 5), (0, 2, 5)):
        for i in c:
            for j in c:
                adj[i, j] = i != j
    assert RR.maximum_cliques(adj) == [(0, 2, 5), (0, 3, 4), (1, 2, 5)]
    assert RR.select_rows(adj).tolist() == [0, 2, 5]


def test_modes_and_gnc_on_the_unfiltered_rows():
    """C = 65 with 40 planted: `kcore` keeps the planted rows; `none` leaves the rejection to GNC-TLS, which takes 54 iterations
    and ends with exactly the 780 planted pairs at weight 1 and every other pair at 0."""
    src, ref, rows, poses = RR.make_fixture(65, 40, 0.01, seed=7)
    k = RR.robust_registration(src, ref, 0.01, inlier_selection='kcore')
    assert np.array_equal(k.selected, rows[0])
    n = RR.robust_registration(src, ref, 0.01, inlier_selection='none')
    RR.check_fixture(n)
    assert n.K == 65 and n.iterations == 54 and len(n.weights) == 65 * 64 // 2
    p, q = RR.pair_rows(65)
    planted = np.isin(p, rows[0]) & np.isin(q, rows[0])
    assert planted.sum() == 780 and np.array_equal(n.weights == 1.0, planted) and np.array_equal(n.weights == 0.0, ~planted)
    assert n.translation_inliers == 40
    for r in (k, n):
        rre, rte = RR.pose_error(r.transform, poses[0])
        assert rre < 0.02 and rte < 0.01


def test_degenerate_inputs_of_the_restatement():
    e = RR.robust_registration(np.zeros((0, 3)), np.zeros((0, 3)))
    assert e.K == 0 and e.valid == 0 and np.array_equal(e.transform, np.eye(4))
    src, ref, rows, _ = RR.make_fixture(65, 20, 0.01, seed=85)
    src[rows[0][3]] = np.nan
    r = RR.robust_registration(src, ref, 0.01)
    assert r.degree[rows[0][3]] == 0 and np.array_equal(r.selected, np.delete(rows[0], 3))
    two = RR.robust_registration(src[rows[0][:2]], ref[rows[0][:2]], 0.01)
    assert two.K == 2 and two.valid == 0 and np.array_equal(two.transform, np.eye(4))


def test_parser_takes_robust_only_as_an_own_method(capsys):
    a = cli.make_parser(own_methods=True).parse_args(['--features-root', 'x', '--method', 'robust', '--noise-bound', '0.3',
                                                      '--inlier-selection', 'kcore', '--num_corr', '250'])
    assert (a.method, a.noise_bound, a.inlier_selection, a.num_corr) == ('robust', 0.3, 'kcore', 250)
    d = cli.make_parser(own_methods=True).parse_args(['--features-root', 'x', '--method', 'robust'])
    assert (d.noise_bound, d.inlier_selection) == (0.01, 'clique')
    assert cli.ROBUST_METHODS == ('robust',) and cli.KERNEL_METHOD['robust'] == 'lgr'
    with pytest.raises(SystemExit):
        cli.make_parser().parse_args(['--features-root', 'x', '--method', 'robust'])
    assert 'robust' in capsys.readouterr().err
    for parser in (cli.make_parser(), cli.make_parser(own_methods=True)):
        with pytest.raises(SystemExit):
            parser.parse_args(['--features-root', 'x', '--method', 'teaser'])
        assert 'teaser' in capsys.readouterr().err
    assert cli.METHODS == ('lgr', 'ransac', 'svd') and cli.OWN_METHODS == ('ransac_featurematch',)
    with pytest.raises(ValueError):
        _lib.EvalOptions.of('robust')  # rdm_eval_options is unchanged: the kernel sees method lgr


def test_host_selection_is_the_documented_rule():
    scores = np.array([0.5, 0.9, 0.5, 0.5, 0.1, 0.9, 0.5], np.float32)
    assert cli.select_rows(scores, 4).tolist() == [0, 1, 2, 5]  # ties: the lowest rows stay
    assert cli.select_rows(scores, 2).tolist() == [1, 5]
    assert cli.select_rows(scores, 7).tolist() == list(range(7)) and cli.select_rows(scores, None).tolist() == list(range(7))
    assert cli.select_rows(scores, 100).tolist() == list(range(7))
    rng = np.random.default_rng(0)
    for _ in range(5):
        s = rng.integers(0, 6, 200).astype(np.float32) / 4 - 0.5  # many ties, negative values
        for L in (1, 17, 199):
            assert np.array_equal(cli.select_rows(s, L), RR.select_num_corr(s, L))


def test_symbols_are_declared_exported_and_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'rdmnet_hip.h')).read()
    L = _lib.lib()
    for n in ('rdm_robust_registration', 'rdm_robust_registration_workspace_bytes', 'rdm_robust_default_clique_nodes'):
        assert re.search(r'\b' + n + r'\s*\(', text) and hasattr(L, n) and n in _lib.SIGNATURES
    assert int(re.search(r'#define RDM_ROBUST_MAX_CORR (\d+)', text).group(1)) == _lib.ROBUST_MAX_CORR
    assert int(re.search(r'#define RDM_ROBUST_STATS (\d+)', text).group(1)) == len(_lib.ROBUST_STATS)
    # host-only: the workspace grows with C, the clique mode adds the search stacks, above the capacity there is none
    sizes = [L.rdm_robust_registration_workspace_bytes(c, 0) for c in (1, 65, 300, 5471, 16384)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < (1 << 30)
    assert L.rdm_robust_registration_workspace_bytes(300, 2) < L.rdm_robust_registration_workspace_bytes(300, 0)
    assert L.rdm_robust_registration_workspace_bytes(16385, 0) == 0
    assert L.rdm_robust_default_clique_nodes() > 0
