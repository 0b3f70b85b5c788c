"""GPU: point-to-point ICP (rdm_icp_point_to_point, rdm_icp_correspondences) against the float64 restatement of
tests/icp_restatement.py, and `python -m rdmnet_amd.prepare` end to end on a KITTI-layout tree.  Open3D (the
reference's implementation) is not in the reference tree: parity is with the restatement only ("unpinned")."""
import os

import numpy as np
import pytest
import torch

import icp_restatement as ir

pytestmark = pytest.mark.gpu

R = 0.5


def cuda32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


def rigid(deg, t, tilt=0.0):
    a = np.deg2rad(tilt)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    T = np.eye(4)
    T[:3, :3] = rot_z(deg) @ Rx
    T[:3, 3] = t
    return T


def raw_pair(seed=0, n_azimuth=2048, step=(1.2, 0.1), yaw=0.4):
    """Two raw 64 x n_azimuth synthetic scans of one scene, in their sensor frames, and the source -> target motion."""
    from rdmnet_amd import synthetic
    rng = np.random.default_rng(seed)
    boxes = synthetic._make_scene(rng)
    tgt = synthetic._scan(boxes, (0.0, 0.0), 0.0, n_azimuth, rng)
    src = synthetic._scan(boxes, step, np.deg2rad(yaw), n_azimuth, rng)
    G = rigid(yaw, [step[0], step[1], 0.0])
    return src, tgt, G


def check_correspondences(pcd, tgt):
    from rdmnet_amd import ops
    idx, d2 = ops.icp_correspondences(torch.from_numpy(pcd).cuda(), cuda32(tgt), R)
    want_idx, want_d2, _ = ir.Target(tgt, R).correspondences(pcd)
    got_idx, got_d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(got_idx, want_idx), int((got_idx != want_idx).sum())
    assert np.array_equal(got_d2.view(np.int64), want_d2.view(np.int64))  # same bits
    return got_idx


@pytest.mark.parametrize('n,m,extent', [(1, 1, 1.0), (5000, 4000, 10.0), (20000, 30000, 40.0), (3000, 100000, 2.0)])
def test_neighbour_step_bit_exact_on_random_clouds(n, m, extent):
    rng = np.random.default_rng(n + m)
    tgt = rng.uniform(-extent, extent, (m, 3)).astype(np.float32)
    pcd = rng.uniform(-extent * 1.1, extent * 1.1, (n, 3))
    got = check_correspondences(pcd, tgt)
    if n > 1:
        assert 0 < (got >= 0).sum() < n or extent <= 2.0


def test_neighbour_step_bit_exact_on_a_raw_size_scan():
    src, tgt, G = raw_pair(1)
    assert len(tgt) > 100000
    pcd = ir.apply(G @ rigid(0.2, [0.05, -0.03, 0.02]), src.astype(np.float64))
    got = check_correspondences(pcd, tgt)
    assert (got >= 0).mean() > 0.5


def test_neighbour_step_bit_exact_on_the_bundled_scans(scans):
    a, b = scans['s000000'], scans['s000004']
    check_correspondences(b.astype(np.float64), a)
    check_correspondences(a.astype(np.float64) + 0.25, b)


def test_neighbour_step_planted_ties_and_radius():
    """Exact ties (mirror images; the larger index in the lower cell) keep the lowest index; d2 == r2 exactly is
    rejected; a query outside the target's box still finds targets within r of the box's edge."""
    q, t = [], []
    for k in range(200):
        c = np.array([3.0 * k - 300.0, 0.75 * (k % 7), -1.5])
        q.append(c)
        e = 0.125 * (1 + k % 3)
        t += [c + [e, 0, 0], c - [e, 0, 0], c + [0, e, 0]]  # three ties at d2 = e^2, their indices in any cell order
        q.append(c + [0, 0, 20.0])
        t.append(c + [0, 0, 20.5])  # d2 == 0.25 == r2 exactly: no correspondence
        t.append(c + [0, 0, 19.5])  # the other one, on the far side, also d2 == r2
    t = np.array(t, np.float32)[::-1].copy()  # larger indices first along x
    q = np.array(q + [[-300.0, -0.45, -1.5], [1e30, 0, 0], [np.nan, 0, 0], [-1e30, -1e30, 5]])  # (the first: one cell below the box)
    idx = check_correspondences(q, t)
    want_tie = len(t) - 1 - np.array([5 * k + 2 for k in range(200)])  # the last written of the three: lowest index now
    assert np.array_equal(idx[0:400:2], want_tie)
    assert (idx[1:400:2] == -1).all()
    assert idx[400] >= 0 and (idx[401:] == -1).all()


def lockstep(source, target, init, max_iteration):
    """Runs the GPU ICP with its history and replays every evaluation in numpy from the GPU's own updates."""
    from rdmnet_amd import ops
    res = ops.icp_point_to_point(cuda32(source), cuda32(target), R, init=init, max_iteration=max_iteration, history=True)
    H = res.history
    assert H.shape == (res.iterations + 1, 15)
    tgt = ir.Target(target, R)
    src = np.asarray(source, np.float32).astype(np.float64)
    pcd = src if init is None else ir.apply(init, src)
    flips = 0
    stop = None
    for k in range(res.iterations + 1):
        idx, d2, near, n, fit, rmse = ir.evaluate(tgt, pcd, len(src))
        n_gpu = int(H[k, 2])
        flips += int(near.sum()) if n != n_gpu else 0
        assert abs(n - n_gpu) <= near.sum(), (k, n, n_gpu, int(near.sum()))
        if n == n_gpu:
            assert abs(fit - H[k, 0]) <= 1e-12 * max(fit, 1e-300) and abs(rmse - H[k, 1]) <= 1e-12 * max(rmse, 1e-300)
        if k < res.iterations:
            ok = idx >= 0
            U = ir.kabsch(pcd[ok], tgt.t[idx[ok]])
            if n == n_gpu:
                assert np.abs(U - H[k, 3:]).max() <= 1e-9, k
            pcd = ir.apply(H[k, 3:], pcd)  # the GPU's own update: errors cannot compound
        if k > 0 and stop is None and abs(H[k - 1, 0] - H[k, 0]) < 1e-6 and abs(H[k - 1, 1] - H[k, 1]) < 1e-6:
            stop = k
    assert res.iterations == (stop if stop is not None else max_iteration)
    assert res.num_correspondences == int(H[-1, 2]) and res.fitness == H[-1, 0] and res.inlier_rmse == H[-1, 1]
    T = np.eye(4) if init is None else np.asarray(init, np.float64)
    for k in range(res.iterations):
        T = ir.compose(H[k, 3:], T)
    assert np.array_equal(T, res.transformation)
    print(f'lock step: {res.iterations} updates, {flips} near-tie points at count differences')
    return res


def test_icp_lockstep_real_scans_from_identity(scans):
    lockstep(scans['s000004'], scans['s000000'], None, 200)


def test_icp_lockstep_synthetic_raw_pair():
    src, tgt, G = raw_pair(2)
    res = lockstep(src, tgt, G @ rigid(0.3, [0.08, -0.05, 0.03]), 100)
    assert res.fitness > 0.5


def test_icp_lockstep_non_identity_init(scans):
    lockstep(scans['s000007'], scans['s000000'], rigid(-1.0, [0.4, 0.2, -0.1], tilt=0.5), 60)


def test_icp_exact_recovery():
    """Source = a subset of a raw target moved by 0.2 deg / 0.15 m (no noise but the float32 storage): the result is
    the inverse motion to 1e-6 m / 1e-6 deg."""
    from rdmnet_amd import ops
    _, tgt, _ = raw_pair(3)
    G = rigid(0.2, [0.12, -0.09, 0.02])
    moved = ir.apply(G, tgt[::3].astype(np.float64))
    res = ops.icp_point_to_point(cuda32(moved), cuda32(tgt), R, max_iteration=500)
    E = res.transformation @ G
    ang = np.rad2deg(np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2)  # (arccos of the trace loses it)
    assert np.abs(E[:3, 3]).max() < 1e-6 and ang < 1e-6, (E, ang)
    assert res.fitness > 0.99 and res.inlier_rmse < 1e-5


def test_icp_exact_recovery_of_a_float32_exact_motion():
    """Source = a target subset moved by a motion that float32 represents exactly (integer-grid points, 90-degree
    turn + cm shift): the inverse comes back to 1e-6 m / 1e-6 degrees."""
    from rdmnet_amd import ops
    rng = np.random.default_rng(4)
    tgt = (rng.integers(-400, 400, (40000, 3)) / 16.0).astype(np.float32)
    tgt = np.unique(tgt, axis=0)
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    sel = tgt[::2].astype(np.float64)
    src = (sel @ Rz.T + [0.125, -0.0625, 0.03125]).astype(np.float32)
    init = np.eye(4)
    init[:3, :3] = Rz.T
    init[:3, 3] = -(Rz.T @ [0.125, -0.0625, 0.03125]) + [0.1, -0.05, 0.02]  # start 0.1 m off
    res = ops.icp_point_to_point(cuda32(src), cuda32(tgt), R, init=init, max_iteration=200)
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rz, [0.125, -0.0625, 0.03125]
    E = res.transformation @ G
    ang = np.rad2deg(np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / 2)  # (arccos of the trace loses it)
    assert np.abs(E[:3, 3]).max() < 1e-6 and ang < 1e-6, (E, ang)


def test_icp_edge_cases():
    from rdmnet_amd import ops
    rng = np.random.default_rng(5)
    tgt = cuda32(rng.uniform(-5, 5, (2000, 3)))
    far = cuda32(rng.uniform(-5, 5, (1500, 3)) + [1000.0, 0, 0])
    # no correspondences: identity update, fitness 0, stops after one update
    res = ops.icp_point_to_point(far, tgt, R, max_iteration=30, history=True)
    assert res.iterations == 1 and res.fitness == 0 and res.num_correspondences == 0 and np.array_equal(res.transformation, np.eye(4))
    assert np.array_equal(res.history[0, 3:], ir.IDENTITY12)
    # empty source returns init
    init = rigid(3.0, [1, 2, 3])
    res = ops.icp_point_to_point(torch.zeros((0, 3), device='cuda'), tgt, R, init=init)
    assert res.iterations == 0 and res.fitness == 0 and np.array_equal(res.transformation, init)
    # empty target: nothing to match
    res = ops.icp_point_to_point(tgt, torch.zeros((0, 3), device='cuda'), R)
    assert res.fitness == 0 and res.iterations == 1
    # max_iteration = 0: init and the initial evaluation
    near = cuda32(tgt.cpu().numpy() + 0.05)
    res = ops.icp_point_to_point(near, tgt, R, init=init, max_iteration=0, history=True)
    assert res.iterations == 0 and np.array_equal(res.transformation, init) and res.history.shape == (1, 15)
    res0 = ops.icp_point_to_point(near, tgt, R, max_iteration=0)
    idx, _ = ops.icp_correspondences(near.double(), tgt, R)
    assert res0.num_correspondences == int((idx >= 0).sum()) > 0
    # max_iteration reached without convergence
    res = ops.icp_point_to_point(near, tgt, R, max_iteration=3, relative_fitness=0.0, relative_rmse=0.0, history=True)
    assert res.iterations == 3 and res.history.shape == (4, 15)
    # source and target far outside each other's box, but within reach at one corner
    a = cuda32(rng.uniform(0, 1, (500, 3)) + [200.0, 200.0, 200.0])
    b = cuda32(np.array([[200.2, 200.2, 200.2]]))
    res = ops.icp_point_to_point(b, a, R, max_iteration=5)
    assert res.num_correspondences == 1
    # a strided source (row stride 4) gives the bits of the contiguous one
    s4 = cuda32(np.concatenate([near.cpu().numpy(), np.ones((near.shape[0], 1))], 1))
    r1 = ops.icp_point_to_point(near, tgt, R, max_iteration=10)
    r2 = ops.icp_point_to_point(s4[:, :3], tgt, R, max_iteration=10)
    assert np.array_equal(r1.transformation, r2.transformation)
    # argument errors
    with pytest.raises(ValueError):
        ops.icp_point_to_point(near, tgt, 0.0)
    bad = tgt.clone()
    bad[7, 1] = float('nan')
    with pytest.raises(RuntimeError, match='not finite'):
        ops.icp_point_to_point(near, bad, R)


def test_icp_is_deterministic():
    from rdmnet_amd import ops
    src, tgt, G = raw_pair(6, n_azimuth=1024)
    init = G @ rigid(0.5, [0.2, 0.1, 0.0])
    a = ops.icp_point_to_point(cuda32(src), cuda32(tgt), R, init=init, max_iteration=100, history=True)
    b = ops.icp_point_to_point(cuda32(src), cuda32(tgt), R, init=init, max_iteration=100, history=True)
    assert np.array_equal(a.transformation, b.transformation) and np.array_equal(a.history, b.history)
    assert a.iterations == b.iterations and a.fitness == b.fitness


# ---- prepare end to end --------------------------------------------------------------------------------------------

TR = np.array([[0.0, -1, 0, -0.004], [0, 0, -1, -0.076], [1, 0, 0, -0.27], [0, 0, 0, 1]])  # velo -> cam, KITTI-like


def drift(k):
    """Known pose error injected into every third frame (camera frame): a few cm and a few tenths of a degree."""
    if k % 3 != 1:
        return np.eye(4)
    D = np.eye(4)
    a = np.deg2rad(0.3)
    D[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]  # yaw about the camera's y
    D[:3, 3] = [0.04, 0.0, -0.03]
    return D


def build_tree(root, n_frames=30, seq=8):
    from rdmnet_amd import synthetic
    rng = np.random.default_rng(7)
    boxes = synthetic._make_scene(rng)
    vel = os.path.join(root, 'sequences', '%02d' % seq, 'velodyne')
    os.makedirs(vel)
    os.makedirs(os.path.join(root, 'poses'))
    os.makedirs(os.path.join(root, 'calib', 'sequences', '%02d' % seq))
    true_poses, lines = [], []
    for k in range(n_frames):
        x, y, yaw = 1.4 * k, 0.05 * k, 0.2 * k
        pts = synthetic._scan(boxes, (x, y), np.deg2rad(yaw), 2048, rng)
        xyzi = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1)
        xyzi.astype(np.float32).tofile(os.path.join(vel, '%06d.bin' % k))
        W = rigid(yaw, [x, y, 0.0])  # velo -> world
        P = TR @ W @ np.linalg.inv(TR)  # the camera-frame pose (T_w_cam0 with the world expressed in cam0 axes)
        true_poses.append(P)
        lines.append(' '.join(f'{v:.12e}' for v in (P @ drift(k))[:3].reshape(-1)))
    with open(os.path.join(root, 'poses', '%02d.txt' % seq), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    with open(os.path.join(root, 'calib', 'sequences', '%02d' % seq, 'calib.txt'), 'w') as f:
        for k in range(4):
            f.write(f'P{k}: ' + ' '.join(['7.0e+02'] + ['0.0'] * 11) + '\n')
        f.write('Tr: ' + ' '.join(f'{v:.12e}' for v in TR[:3].reshape(-1)) + '\n')
    return true_poses


def test_prepare_end_to_end(tmp_path):
    from oracle import preprocess
    from rdmnet_amd import dataset, prepare
    root = str(tmp_path)
    true_poses = build_tree(root)
    assert prepare.main(['downsample', '--dataset-root', root, '--sequences', '8']) == 0
    for k in (0, 13, 29):
        raw = prepare.read_scan(root, 8, k)
        got = np.load(os.path.join(root, 'downsampled_xyzi', '08', '%06d.npy' % k))
        assert got.dtype == np.float32 and np.array_equal(got, preprocess.voxel_down_sample(raw, 0.3))
    assert prepare.main(['pairs', '--dataset-root', root, '--sequences', '8']) == 0
    poses = prepare.read_poses(os.path.join(root, 'poses', '08.txt'))
    velo2cam = prepare.read_velo2cam(os.path.join(root, 'calib', 'sequences', '08', 'calib.txt'))
    want_pairs = prepare.pair_frames(range(30), poses[:, :3, 3], 10)
    items = dataset.load_kitti_gt_txt(os.path.join(root, 'icp10'), 8)
    assert [(d['frame1'], d['frame0']) for d in items] == want_pairs and len(want_pairs) >= 2
    for (curr, nxt), d in zip(want_pairs, items):
        M = prepare.relative_transform(velo2cam, poses[curr], poses[nxt])
        src, tgt = prepare.read_scan(root, 8, curr)[:, :3], prepare.read_scan(root, 8, nxt)[:, :3]
        T_ref, fit, _, _, it = ir.icp(src, tgt, 0.5, init=M, max_iteration=5000)
        assert np.abs(d['transform'] - T_ref).max() <= 1e-6 + 5e-7  # (+ the file's 6 decimals)
        # drift removal: the true velo(curr) -> velo(next) motion
        G = np.linalg.inv(TR) @ np.linalg.inv(true_poses[nxt]) @ true_poses[curr] @ TR
        err_odo = np.abs(M - G).max()
        err_icp = np.abs(d['transform'] - G).max()
        err_ref = np.abs(T_ref - G).max()
        # the bound is the restatement's own residual on this data (+ the file's rounding): what ICP can do here
        assert err_icp <= err_ref + 1e-6, (curr, nxt, err_odo, err_ref, err_icp)
        if err_odo > 0.01:  # a drifted pair: the refined pose is closer to the truth than the odometry
            assert err_icp < err_odo, (curr, nxt, err_odo, err_icp)
        print(f'pair {curr}->{nxt}: {it} updates, fitness {fit:.3f}, odometry error {err_odo:.4f}, ICP error {err_icp:.4f}')
    for seq in (9, 10):  # the test split's other sequences: no scans in this tree, empty pair lists
        open(os.path.join(root, 'icp10', '%02d' % seq), 'w').close()
    ds = dataset.OdometryKittiPairDataset(root, 'test')
    assert len(ds) == len(want_pairs)
    item = ds[0]
    assert item['ref_points'].shape[1] == 3 and item['transform'].shape == (4, 4)
