"""GPU: ops.robust_registration (rdm_robust_registration), `eval --method robust` and `infer --robust` against the float64
restatement tests/robust_restatement.py.

Graph stage, selection, iteration counts, translation inliers and (on these fixtures, where every final weight is 0 or 1) the
weights are compared exactly: the restatement asserts on every fixture that no pair lies within 1e-9 of the compatibility
threshold, that the maximum clique is unique (unless the case is about ties) and that the best translation cost of an axis is
more than 1e-9 relative below the next.

Pose tolerance.  Fixed-order float64 sums of K^2 / 2 terms differ from numpy's pairwise sums by a few ulp of the sum, and the Horn
solve amplifies that; the bound is therefore 10 x the restatement's own spread under 20 random orders of the measurement pairs,
measured by the test on each fixture (robust_restatement.permutation_spread) and printed beside the differences.  Measured
spreads (largest rotation entry / translation entry / weight), so bounds of ten times these:
    (65, 20, 0.01)    7.8e-16 / 6.7e-15 / 0        (129, 40, 0.01)   2.7e-15 / 6.2e-15 / 0
    (300, 120, 0.01)  3.8e-15 / 4.7e-15 / 0        (300, 60, 0.05)   1.3e-15 / 8.1e-15 / 0
    (65, 40, 0.01) none: 2.4e-15 / 8.0e-15 / 0, 54 iterations in every order;  kcore: 2.9e-15 / 9.3e-15 / 0
    two groups: 8.9e-16 / 1.1e-14 / 0;  NaN row: 1.1e-15 / 1.0e-14 / 0;  duplicate row: 7.8e-16 / 1.0e-14 / 0
    200 random rows at 0.3: 1.1e-15 / 1.8e-15 / 0, 23 iterations in every order
On one MI355X the differences from the restatement were 2.8e-16 to 2.4e-15 (rotation) and 3.1e-16 to 6.7e-15 (translation), each
below its fixture's spread, the weights and the iteration counts equal.  The GNC iteration count may differ by one from the
restatement's."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import robust_restatement as RR

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_KEYS = ('ref_points_c', 'src_points_c', 'ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points',
             'src_corr_points', 'corr_scores', 'gt_node_corr_indices', 'gt_node_corr_overlaps', 'transform', 'estimated_transform')
_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def run(ops, src, ref, beta, **kw):
    return ops.robust_registration(dev(src), dev(ref), noise_bound=beta, return_weights=True, return_graph=True, **kw)


def planted(C, n_in, beta, seed, mode='clique'):
    """(src, ref, rows, poses, restated result), computed once per fixture and left unchanged."""
    key = (C, n_in, beta, seed, mode)
    if key not in _cache:
        src, ref, rows, poses = RR.make_fixture(C, n_in, beta, seed=seed)
        res = RR.robust_registration(src, ref, beta, inlier_selection=mode)
        RR.check_fixture(res)
        _cache[key] = (src, ref, rows, poses, res)
    return _cache[key]


def same_graph(got, want, where=''):
    assert np.array_equal(got.degree, want.degree), where
    assert np.array_equal(got.core, want.core), where
    assert got.edges == want.edges, where
    assert np.array_equal(got.selected, want.selected), where
    assert (got.num_selected, got.valid) == (want.K, want.valid), where


def same_pose(got, want, src, ref, beta, where=''):
    dR, dt, dw, its = RR.permutation_spread(src, ref, want, noise_bound=beta)
    eR = np.abs(got.transformation[:3, :3] - want.transform[:3, :3]).max()
    et = np.abs(got.transformation[:3, 3] - want.transform[:3, 3]).max()
    ew = np.abs(got.weights - want.weights).max()
    print(where, 'rotation', eR, 'spread', dR, '| translation', et, 'spread', dt, '| weights', ew, 'spread', dw, '| iterations',
          got.iterations, want.iterations, its)
    assert got.weights.shape == want.weights.shape
    assert eR <= 10 * dR and et <= 10 * dt and ew <= 10 * dw, where
    assert abs(got.iterations - want.iterations) <= 1, where
    assert got.translation_inliers == want.translation_inliers, where
    assert np.array_equal(got.transformation[3], [0, 0, 0, 1])


@pytest.mark.parametrize('C', [1, 2, 3, 63, 64, 65, 129, 300])
def test_graph_stage_equals_the_restatement(ops, C):
    """Word and wave boundaries.  A third of the rows is planted (all of them up to C = 3), beta 0.05.  The pose is compared on
    the pose fixtures (a sum of three terms has no spread to derive a bound from)."""
    n_in = max(C // 3, min(C, 3))
    src, ref, rows, poses, want = planted(C, n_in, 0.05, 1000 + C)
    got = run(ops, src, ref, 0.05)
    same_graph(got, want, f'C={C}')
    assert got.exact == 1
    assert got.translation_inliers == want.translation_inliers and got.iterations == want.iterations
    if want.K >= 20:
        rre, rte = RR.pose_error(got.transformation, poses[0])
        assert rre < 0.02 and rte < 0.05  # (tests/test_robust.py: the planted pose)
    if not want.valid:
        assert np.array_equal(got.transformation, np.eye(4))


@pytest.mark.parametrize('C,n_in,beta', [(65, 20, 0.01), (129, 40, 0.01), (300, 120, 0.01), (300, 60, 0.05)])
def test_pose_equals_the_restatement(ops, C, n_in, beta):
    src, ref, rows, poses, want = planted(C, n_in, beta, C + n_in)
    got = run(ops, src, ref, beta)
    same_graph(got, want)
    assert np.array_equal(got.selected, rows[0]) and got.exact == 1
    same_pose(got, want, src, ref, beta, f'{(C, n_in, beta)}')
    rre, rte = RR.pose_error(got.transformation, poses[0])
    assert rre < 0.02 and rte < beta  # (tests/test_robust.py: the planted pose)


def test_two_equal_groups_the_lower_first_row_wins_bit_equal_twice(ops):
    src, ref, rows, poses = RR.make_fixture(129, 30, 0.01, seed=11, groups=2)
    want = RR.robust_registration(src, ref, 0.01)
    RR.check_fixture(want, unique_clique=False)
    assert len(RR.maximum_cliques(want.adjacency)) == 2
    a, b = run(ops, src, ref, 0.01), run(ops, src, ref, 0.01)
    same_graph(a, want)
    assert np.array_equal(a.selected, min(rows, key=lambda r: r[0])) and a.exact == 1
    same_pose(a, want, src, ref, 0.01, 'tie')
    for name in ('transformation', 'selected', 'weights', 'degree', 'core'):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert repr(a) == repr(b)


@pytest.mark.parametrize('mode', ['kcore', 'none'])
def test_kcore_and_none_modes(ops, mode):
    """C = 65 with 40 planted.  `none` exercises GNC: 54 iterations in the restatement, exactly the 780 planted pairs at 1."""
    src, ref, rows, poses, want = planted(65, 40, 0.01, 7, mode)
    got = run(ops, src, ref, 0.01, inlier_selection=mode)
    same_graph(got, want, mode)
    same_pose(got, want, src, ref, 0.01, mode)
    if mode == 'none':
        assert want.iterations == 54 and got.num_selected == 65
        assert (got.weights == 1.0).sum() == 780 and (got.weights == 0.0).sum() == 65 * 64 // 2 - 780
    else:
        assert np.array_equal(got.selected, rows[0])


def test_degenerate_inputs(ops):
    import torch
    empty = ops.robust_registration(torch.zeros((0, 3), device='cuda'), torch.zeros((0, 3), device='cuda'), return_graph=True)
    assert (empty.num_selected, empty.valid, empty.exact, empty.iterations, empty.translation_inliers, empty.edges) == (0, 0, 1, 0, 0, 0)
    assert np.array_equal(empty.transformation, np.eye(4)) and len(empty.selected) == 0
    src, ref, rows, poses = RR.make_fixture(65, 20, 0.01, seed=85)
    # K < 3: two compatible rows
    two = run(ops, src[rows[0][:2]], ref[rows[0][:2]], 0.01)
    assert (two.num_selected, two.valid, two.edges) == (2, 0, 1) and np.array_equal(two.transformation, np.eye(4))
    assert two.selected.tolist() == [0, 1] and two.degree.tolist() == [1, 1] and two.core.tolist() == [1, 1]
    # a NaN row is adjacent to nothing and leaves the clique
    s2 = src.copy()
    s2[rows[0][3], 1] = np.nan
    want = RR.robust_registration(s2, ref, 0.01)
    RR.check_fixture(want)
    got = run(ops, s2, ref, 0.01)
    same_graph(got, want, 'nan')
    assert got.degree[rows[0][3]] == 0 and rows[0][3] not in got.selected and got.num_selected == 19
    same_pose(got, want, s2, ref, 0.01, 'nan')
    # duplicate rows: the copy of a planted row is compatible with the whole group and with its original (both distances are 0)
    s3, r3 = np.concatenate([src, src[rows[0][:1]]]), np.concatenate([ref, ref[rows[0][:1]]])
    want = RR.robust_registration(s3, r3, 0.01)
    RR.check_fixture(want)
    assert want.K == 21 and want.selected[-1] == 65
    got = run(ops, s3, r3, 0.01)
    same_graph(got, want, 'duplicate')
    same_pose(got, want, s3, r3, 0.01, 'duplicate')
    # above the capacity: the error code, nothing launched
    from rdmnet_amd import _lib
    big = torch.zeros((_lib.ROBUST_MAX_CORR + 1, 3), device='cuda')
    with pytest.raises(RuntimeError, match=r'code -4.*16385'):
        ops.robust_registration(big, big)


def test_search_budget(ops):
    """200 random rows in a +-2 m box at beta 0.3: density 0.32, one maximum clique of 11.  16 nodes per subproblem are not enough:
    exact = 0, still a clique of the graph, the same on a second run; the default budget finishes the search."""
    rng = np.random.default_rng(0)
    src, ref = rng.uniform(-2, 2, (200, 3)).astype(np.float32), rng.uniform(-2, 2, (200, 3)).astype(np.float32)
    want = RR.robust_registration(src, ref, 0.3)
    RR.check_fixture(want)
    assert want.K == 11 and 0.30 < want.edges / (200 * 199 / 2) < 0.33
    small = [run(ops, src, ref, 0.3, max_clique_nodes=16) for _ in range(2)]
    for r in small:
        assert r.exact == 0 and 3 <= r.num_selected <= 11 and np.array_equal(r.degree, want.degree)
        rows = r.selected
        assert np.all(np.diff(rows) > 0) and want.adjacency[np.ix_(rows, rows)].sum() == len(rows) * (len(rows) - 1)
    for name in ('transformation', 'selected', 'weights'):
        assert getattr(small[0], name).tobytes() == getattr(small[1], name).tobytes(), name
    full = run(ops, src, ref, 0.3)
    assert full.exact == 1
    same_graph(full, want, 'budget')
    same_pose(full, want, src, ref, 0.3, 'budget')


def test_eval_command_line(ops, golden_dir, tmp_path, capsys):
    """`eval --method robust --noise-bound 0.3 --num_corr 250` on the golden pair files.  The fixture's poses and correspondences
    come from seeded random weights, so no pair is expected to be accepted and recall is not asserted: the transforms are those of
    ops.robust_registration on the host-selected rows, bit for bit, and the records are evaluate_pairs('lgr') given them."""
    from rdmnet_amd import eval as cli
    z = np.load(os.path.join(golden_dir, 'eval_pairs.npz'))
    names = [str(n) for n in z['names']]
    pairs = {n: {k: z[f'{n}/{k}'] for k in FILE_KEYS} for n in names}
    for n in names:
        np.savez_compressed(tmp_path / (n + '.npz'), **pairs[n])
    args = cli.make_parser(own_methods=True).parse_args(['--features-root', str(tmp_path), '--method', 'robust', '--noise-bound', '0.3',
                                                         '--num_corr', '250', '--batch', '3', '--test_epoch', '1'])
    got = []
    cli.evaluate(args, collect=got)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'Epoch 1, method robust' and len(out) == 5 and out[4].startswith('  Registration, RR: ')
    assert len(got) == len(names)
    order = [os.path.basename(f)[:-4] for _, f, _ in cli.list_pairs(str(tmp_path))[1]]
    est = {}
    for n, (ids, rec, used) in zip(order, got):
        d = pairs[n]
        rows = RR.select_num_corr(d['corr_scores'], 250)
        assert len(rows) == 250
        res = ops.robust_registration(dev(d['src_corr_points'][rows]), dev(d['ref_corr_points'][rows]), noise_bound=0.3)
        est[n] = res.transformation.astype(np.float32)
        assert used.tobytes() == est[n].tobytes(), n
        assert res.valid == 1 and res.num_selected >= 3
    records, _ = ops.evaluate_pairs([dict(pairs[n], estimated_transform=est[n]) for n in order], 'lgr', 250)
    assert np.array_equal(records, np.stack([rec for _, rec, _ in got]), equal_nan=True)


def test_harness_adds_one_key(tmp_path):
    runs = {}
    for name, flags in (('plain', []), ('robust', ['--robust', '--noise-bound', '0.1'])):
        out_dir = tmp_path / name
        cmd = [sys.executable, '-m', 'rdmnet_amd.infer', '--synthetic', '2', '--synthetic-distinct', '2', '--synthetic-cache',
               str(tmp_path / 'pairs'), '--out', str(out_dir), '--pairs-in-flight', '1', '--no-ransac'] + flags
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        files = sorted(glob.glob(str(out_dir / '*.npz')))
        assert len(files) == 2
        runs[name] = ([dict(np.load(fn)) for fn in files], [x for x in p.stdout.splitlines() if x.startswith('seq_id')])
    for plain, with_r, line, plain_line in zip(runs['plain'][0], runs['robust'][0], runs['robust'][1], runs['plain'][1]):
        assert set(with_r) == set(plain) | {'estimated_transform_robust'} and 'estimated_transform_robust' not in plain
        for k in plain:
            assert np.array_equal(plain[k], with_r[k]), k
        T = with_r['estimated_transform_robust']
        assert T.dtype == np.float64 and T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1])
        assert line.startswith(plain_line + ', robust_K: ') and 'robust_exact: ' in line and 'robust' not in plain_line
        if 'transform' in with_r:
            assert 'robust_RRE: ' in line and 'robust_RTE: ' in line
