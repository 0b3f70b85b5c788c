"""rdmnet_amd.trajectory on the host: the reference's chaining, Umeyama alignment and absolute trajectory error against
tests/golden/trajectory.npz (written by tests/golden/gen_trajectory_golden.py from the reference's own functions), and the
command line without --optimize."""
import os

import numpy as np
import pytest

from rdmnet_amd import trajectory

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'trajectory.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cases(golden):
    return range(int(golden['n_cases']))


def test_chain_poses_equals_the_reference(golden):
    for k in cases(golden):
        for pair, traj in ((f'pair_{k}', f'traj_{k}'), (f'gt_pair_{k}', f'gt_traj_{k}')):
            got = trajectory.chain_poses(golden[pair])
            assert got.shape == golden[traj].shape
            np.testing.assert_allclose(got, golden[traj], rtol=0, atol=1e-12)


def test_umeyama_alignment_equals_the_reference(golden):
    for k in cases(golden):
        x, y = golden[f'traj_{k}'][:, :3, 3].T, golden[f'gt_traj_{k}'][:, :3, 3].T
        r, t, c = trajectory.umeyama_alignment(x, y)
        want = golden[f'umeyama_{k}']
        np.testing.assert_allclose(np.concatenate([r.reshape(-1), t, [c]]), want, rtol=0, atol=1e-12)


def test_absolute_trajectory_error_equals_the_reference(golden):
    for k in cases(golden):
        err = trajectory.absolute_trajectory_error(golden[f'traj_{k}'], golden[f'gt_traj_{k}'])
        got = np.array([err[key] for key in trajectory.REFERENCE_KEYS])
        assert np.array_equal(got, golden[f'errors_{k}']), (k, got, golden[f'errors_{k}'])  # the rounded keys: exactly
        u = err['unrounded']
        want = golden[f'unrounded_{k}']  # mean, rmse (metres), mean angle, rotation RMSE (degrees)
        np.testing.assert_allclose([u['mean'], u['rmse'], u['r_mean'], u['rotation_rmse_deg']], want, rtol=0,
                                   atol=1e-12)
        assert u['r_rmse'] == u['rmse']  # the reference's r_rmse is the root of the TRANSLATION mean square
        assert err['r_rmse'] == round(u['rmse'], 2) and err['rotation_rmse_deg'] == round(u['rotation_rmse_deg'], 2)


def test_a_trajectory_equal_to_its_ground_truth_has_no_error(golden):
    k = max(cases(golden))
    assert np.array_equal(golden[f'pair_{k}'], golden[f'gt_pair_{k}'])
    err = trajectory.absolute_trajectory_error(golden[f'traj_{k}'], golden[f'gt_traj_{k}'])
    assert [err[key] for key in trajectory.REFERENCE_KEYS] == [0.0, 0.0, 0.0, 0.0]


# ---- the command line ------------------------------------------------------------------------------------------------------

def write_pairs(root, seq, frames, est, gt, information=True, loops=()):
    """Pair k: src = frames[k], ref = frames[k + 1]; loops: (src frame, ref frame, transform)."""
    for k in range(len(est)):
        d = dict(estimated_transform=est[k], transform=gt[k])
        if information:
            d['information'] = np.eye(6) * (k + 1)
        np.savez(os.path.join(root, f'{seq}_{frames[k]}_{frames[k + 1]}.npz'), **d)
    for src, ref, T in loops:
        np.savez(os.path.join(root, f'{seq}_{src}_{ref}.npz'), estimated_transform=T, transform=T, information=np.eye(6))


def run_cli(argv):
    lines = []
    args = trajectory.make_parser().parse_args(argv)
    trajectory.run(args, emit=lines.append)
    return lines


def test_cli_reports_the_chained_trajectory(golden, tmp_path):
    root, out = tmp_path / 'pairs', tmp_path / 'traj'
    root.mkdir()
    n = 10
    write_pairs(str(root), 9, list(range(0, 10 * (n + 1), 10)), golden['pair_1'], golden['gt_pair_1'])
    write_pairs(str(root), 10, list(range(5, 5 + 3 * 4, 3)), golden['pair_0'], golden['gt_pair_0'])
    lines = run_cli(['--features-root', str(root), '--out', str(out)])
    want = []
    for seq, k in ((9, 1), (10, 0)):
        e = golden[f'errors_{k}']
        rot = round(float(golden[f'unrounded_{k}'][3]), 2)
        want.append(f'seq {seq} chained: r_rmse: {e[0]}, r_mean: {e[1]}, rmse: {e[2]}, mean: {e[3]}, rotation_rmse_deg: {rot}')
    assert lines == want
    poses = np.loadtxt(str(out / '9_chained.txt'))
    assert poses.shape == (n + 1, 12)  # one pose per frame: the first frame (the identity) and the chained poses
    np.testing.assert_array_equal(poses[0].reshape(3, 4), np.eye(4)[:3])
    np.testing.assert_allclose(poses[1:].reshape(n, 3, 4), golden['traj_1'][:, :3], rtol=0, atol=1e-7)
    assert (out / '10_chained.txt').exists() and not (out / '9_optimized.txt').exists()


def test_cli_names_a_file_without_information(golden, tmp_path):
    write_pairs(str(tmp_path), 9, [0, 10, 20, 30], golden['pair_0'], golden['gt_pair_0'], information=False)
    with pytest.raises(trajectory.TrajectoryError, match=r'9_0_10\.npz.*infer --information'):
        run_cli(['--features-root', str(tmp_path)])
    assert len(run_cli(['--features-root', str(tmp_path), '--unit-information'])) == 1
    with pytest.raises(SystemExit, match='infer --information'):
        trajectory.main(['--features-root', str(tmp_path)])


def test_cli_names_a_frame_outside_the_chain(golden, tmp_path):
    write_pairs(str(tmp_path), 9, [0, 10, 20, 30], golden['pair_0'], golden['gt_pair_0'], loops=[(7, 10, np.eye(4))])
    with pytest.raises(trajectory.TrajectoryError, match=r'9_7_10\.npz: frame 7 of sequence 9'):
        run_cli(['--features-root', str(tmp_path)])


def test_sequence_graph_links_the_chain_and_marks_the_loops(golden, tmp_path):
    loop = np.linalg.inv(golden['pair_0'][0]) @ np.eye(4)
    write_pairs(str(tmp_path), 9, [0, 10, 20, 30], golden['pair_0'], golden['gt_pair_0'], loops=[(30, 10, loop)])
    seqs = trajectory.read_sequences(str(tmp_path))
    nodes, edges, transforms, infos, uncertain, names = trajectory.sequence_graph(seqs[9])
    assert seqs[9]['frames'] == [0, 10, 20, 30]
    assert edges.tolist() == [[0, 1], [1, 2], [2, 3], [3, 1]] and uncertain.tolist() == [0, 0, 0, 1]
    assert names == ['9_0_10.npz', '9_10_20.npz', '9_20_30.npz', '9_30_10.npz']
    np.testing.assert_array_equal(nodes[0], np.eye(4))
    np.testing.assert_allclose(nodes[1:], golden['traj_0'], rtol=0, atol=1e-12)
    for (s, t), T in zip(edges[:3], transforms[:3]):  # the chained nodes satisfy the model X_s = X_t T on the chain
        np.testing.assert_allclose(nodes[s], nodes[t] @ T, rtol=0, atol=1e-12 * np.abs(nodes).max())
    assert infos.shape == (4, 6, 6)


def test_cli_optimize_without_pair_files_says_so(tmp_path):
    with pytest.raises(trajectory.TrajectoryError, match='no pair files'):
        run_cli(['--features-root', str(tmp_path), '--optimize'])
