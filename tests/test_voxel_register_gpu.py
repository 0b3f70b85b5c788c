"""GPU: the scan-to-map registration (rdm_voxel_map_register, ops.VoxelMap.register, `trajectory --map-refine`) against the NumPy
restatement tests/voxel_register_restatement.py on the street of test_voxel_register: the evaluation alone within the worst-case
summation bound, a fixed number of updates, bit equality across runs, batch positions, capacities and integration orders, the
edge cases, the raw C-ABI's argument errors, recovery of a perturbed pose, and one command-line run.

Scans of 4 000 points; maps of seven scans under their true poses at 0.3 m and 1 m voxels, straddling the origin (negative cells in x
and y); the registered scan is the eighth (index 4), which the maps do not hold."""
import os

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_register_restatement as RR
from test_voxel_register import perturb, pose_error, street

pytestmark = pytest.mark.gpu

VOXELS = (0.3, 1.0)
SIGMA = 0.02
ERR_ARG, ERR_WORKSPACE = -1, -2  # RDM_ERR_ARG, RDM_ERR_WORKSPACE
# The largest entry-wise difference between the library's pose and the restatement's after five updates, measured over the eight
# cases of test_five_updates_agree_with_the_restatement: 1.8e-15 (rotation entries and metres alike).  Rounding of the differently
# ordered sums, carried through five solves.  The asserted bound is 100 times that (the margin is for a point within rounding of a
# cell face that takes the other voxel in one of the two computations), far below the cap of 1e-9.
POSE_MEASURED = 1.8e-15
POSE_BOUND = 100.0 * POSE_MEASURED
_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def scene():
    """Computed once, never changed: the clouds, the true poses, per voxel size the restatement's map of the seven other scans."""
    if 'scene' not in _cache:
        clouds, poses = street(np.random.default_rng(5), per_scan=4000)
        others = [k for k in range(len(clouds)) if k != 4]
        tables = {v: MR.build([clouds[k] for k in others], poses[others], v, 3) for v in VOXELS}
        _cache['scene'] = (clouds, poses, others, tables)
    return _cache['scene']


def gpu_map(ops, voxel, order=None, capacity=1 << 16):
    import torch
    clouds, poses, others, _ = scene()
    order = others if order is None else order
    return ops.VoxelMap(voxel, channels=3, capacity=capacity, moments=True).integrate([torch.from_numpy(clouds[k]).cuda() for k in order],
                                                                                    poses[order])


def shared_map(ops, voxel):
    if ('map', voxel) not in _cache:
        _cache['map', voxel] = gpu_map(ops, voxel)
    return _cache['map', voxel]


def starts(seeds=(3, 4), sigma_t=0.05, sigma_r=0.005):
    _, poses, _, _ = scene()
    return np.stack([perturb(poses[4], np.random.default_rng(s), sigma_t, sigma_r) for s in seeds])


def outputs(res):
    return (res.transformations, res.information, res.gradient, res.cost, res.iterations, res.num_correspondences, res.num_points, res.status)


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    import torch
    return all(torch.equal(x[rows_a], y[rows_b]) for x, y in zip(outputs(a), outputs(b)))


def cuda(cloud):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).cuda()


# ---- the evaluation alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
def test_evaluation_is_within_the_summation_bound(ops, voxel, neighbors):
    """max_iteration = 0.  Counts exactly; every entry of cost, g and H within 2^-52 (n_corr + 64 kappa) A of the restatement's, A =
    the restatement's sum of the absolute values of that entry's terms, kappa = (voxel^2 + sigma^2) / sigma^2: the worst case of
    a sum of n_corr terms in another order, plus the differently ordered 3 x 3 inverse.  Measured: the largest ratio to the bound over
    the four cases is 7.7e-4."""
    clouds, poses, _, tables = scene()
    X = np.concatenate([starts(), poses[4:5]])
    res = shared_map(ops, voxel).register([cuda(clouds[4])] * 3, X, sigma=SIGMA, neighbors=neighbors, max_iteration=0)
    assert res.status.tolist() == [0, 0, 0] and res.iterations.tolist() == [0, 0, 0]
    assert np.array_equal(res.transformations.cpu().numpy(), X)
    H, g, cost = res.information.cpu().numpy(), res.gradient.cpu().numpy(), res.cost.cpu().numpy()
    kappa = (voxel ** 2 + SIGMA ** 2) / SIGMA ** 2
    worst = 0.0
    for s in range(3):
        e = RR.evaluate(tables[voxel], clouds[4], X[s], SIGMA, 4, neighbors)
        assert int(res.num_correspondences[s]) == e['n_corr'] and int(res.num_points[s]) == e['n_points'] == len(clouds[4])
        assert e['n_corr'] > 300
        bound = 2.0 ** -52 * (e['n_corr'] + 64.0 * kappa)
        ratios = [np.abs(H[s] - e['H']) / (bound * e['abs_H']), np.abs(g[s] - e['g']) / (bound * e['abs_g']),
                  np.abs(cost[s] - e['cost']) / (bound * e['abs_cost'])]
        worst = max([worst] + [float(np.max(r)) for r in ratios])
        assert all(np.max(r) <= 1.0 for r in ratios), (s, [float(np.max(r)) for r in ratios])
        assert np.array_equal(H[s], H[s].T)
    print(f'voxel {voxel}, neighbors {neighbors}: largest |difference| / bound = {worst:.3e}')


# ---- a fixed number of updates ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
def test_five_updates_agree_with_the_restatement(ops, voxel, neighbors):
    clouds, _, _, tables = scene()
    X = starts()
    res = shared_map(ops, voxel).register([cuda(clouds[4])] * 2, X, sigma=SIGMA, neighbors=neighbors, max_iteration=5, rot_eps=0.0,
                                          trans_eps=0.0)
    assert res.status.tolist() == [0, 0] and res.iterations.tolist() == [5, 5]
    T = res.transformations.cpu().numpy()
    for s in range(2):
        want = RR.register(tables[voxel], clouds[4], X[s], SIGMA, 4, neighbors, 5, 0.0, 0.0)
        assert want['status'] == 0 and want['iterations'] == 5
        diff = float(np.abs(T[s] - want['transform']).max())
        print(f'voxel {voxel}, neighbors {neighbors}, start {s}: largest pose difference {diff:.3e}')
        assert diff <= POSE_BOUND <= 1e-9
        assert int(res.num_correspondences[s]) == want['n_corr']
        assert T[s, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


# ---- bit equality ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
def test_runs_batch_positions_and_an_empty_scan_do_not_change_a_bit(ops, neighbors):
    import torch
    clouds, poses, _, _ = scene()
    vmap = shared_map(ops, 0.3)
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=neighbors, max_iteration=6)
    alone = vmap.register([cuda(clouds[4])], X[:1], **kw)
    assert same(alone, vmap.register([cuda(clouds[4])], X[:1], **kw))
    assert int(alone.iterations[0]) >= 1 and int(alone.num_correspondences[0]) > 300
    empty = torch.zeros((0, 3), dtype=torch.float32, device='cuda')
    batch = [cuda(clouds[2]), empty, cuda(clouds[4]), cuda(clouds[6][:1000]), cuda(clouds[4]), empty]
    Xb = np.stack([poses[2], np.eye(4), X[0], poses[6], X[0], X[1]])
    both = vmap.register(batch, Xb, **kw)
    assert same(both, vmap.register(batch, Xb, **kw))
    assert same(alone, both, rows_b=slice(2, 3)) and same(alone, both, rows_b=slice(4, 5))
    first = vmap.register([cuda(clouds[4]), cuda(clouds[1])], np.stack([X[0], poses[1]]), **kw)
    assert same(alone, first, rows_b=slice(0, 1))
    # an empty scan is degenerate where it stands and moves nothing
    assert both.status[[1, 5]].tolist() == [2, 2] and both.num_points[[1, 5]].tolist() == [0, 0]
    assert np.array_equal(both.transformations[[1, 5]].cpu().numpy(), Xb[[1, 5]])


def near(cloud, n):
    return cloud[np.argsort(np.linalg.norm(cloud, axis=1), kind='stable')[:n]]


def test_capacity_and_growth_do_not_change_a_bit(ops):
    clouds, poses, _, _ = scene()
    part = near(clouds[3], 1500)
    query, X = cuda(near(clouds[4], 1500)), starts()
    small = ops.VoxelMap(1.0, channels=3, capacity=1 << 12, moments=True).integrate([cuda(part)], poses[3:4])
    assert small.capacity == 1 << 12
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4)
    before = small.register([query, query], X, **kw)
    assert int(before.num_correspondences.min()) > 300
    small._reserve(28000)  # what a batch of 28 000 points would make integrate do
    assert small.capacity == 1 << 16
    assert same(before, small.register([query, query], X, **kw))
    large = ops.VoxelMap(1.0, channels=3, capacity=1 << 16, moments=True).integrate([cuda(part)], poses[3:4])
    assert same(before, large.register([query, query], X, **kw))


def test_the_order_of_integration_does_not_change_a_bit(ops):
    clouds, _, others, _ = scene()
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4)
    a = shared_map(ops, 1.0).register([cuda(clouds[4])] * 2, X, **kw)
    b = gpu_map(ops, 1.0, order=others[::-1], capacity=1 << 17).register([cuda(clouds[4])] * 2, X, **kw)
    assert same(a, b)


# ---- edge cases ------------------------------------------------------------------------------------------------------------------

def test_a_scan_far_from_the_map_is_degenerate_and_keeps_its_pose(ops):
    clouds, poses, _, _ = scene()
    X = poses[4].copy()
    X[:3, 3] += [1000.0, -2000.0, 50.0]
    res = shared_map(ops, 0.3).register([cuda(clouds[4])], X[None], neighbors=7)
    assert res.status.tolist() == [2] and res.num_correspondences.tolist() == [0] and res.iterations.tolist() == [0]
    assert res.num_points.tolist() == [len(clouds[4])]
    assert np.array_equal(res.transformations[0].cpu().numpy(), X)
    assert not res.information.any() and not res.gradient.any() and not res.cost.any()
    assert 'degenerate after 0 updates, 0 correspondences' in repr(res)


def test_min_points_boundary(ops):
    """Voxel (0, 0, 0) of a 1 m map holds three points and voxel (-2, 1, 0) four: with min_points = 4 only the second takes part,
    with 3 both do, with 5 neither."""
    rng = np.random.default_rng(8)
    cloud = np.concatenate([rng.uniform(0.2, 0.8, (3, 3)), rng.uniform(0.2, 0.8, (4, 3)) + [-2.0, 1.0, 0.0]]).astype(np.float32)
    vmap = ops.VoxelMap(1.0, channels=3, capacity=64, moments=True).integrate([cuda(cloud)], np.eye(4)[None])
    table = MR.build([cloud], [np.eye(4)], 1.0, 3)
    query = np.float32([[0.5, 0.5, 0.5], [-1.5, 1.5, 0.5], [7.5, 7.5, 7.5]])
    for least, want in ((3, 2), (4, 1), (5, 0)):
        res = vmap.register([cuda(query)], np.eye(4)[None], min_points=least, max_iteration=0)
        e = RR.evaluate(table, query, np.eye(4), 0.02, least, 1)
        assert res.num_correspondences.tolist() == [want] == [e['n_corr']] and res.num_points.tolist() == [3]
        assert abs(float(res.cost[0]) - e['cost']) <= 2.0 ** -52 * (want + 64.0 * (1.0 + 0.02 ** 2) / 0.02 ** 2) * e['abs_cost']
    # the six neighbours: the point of cell (1, 0, 0) sees voxel (0, 0, 0) through its -x neighbour only
    res = vmap.register([cuda(np.float32([[1.5, 0.5, 0.5]]))], np.eye(4)[None], min_points=3, neighbors=7, max_iteration=0)
    assert res.num_correspondences.tolist() == [1]
    assert vmap.register([cuda(np.float32([[1.5, 0.5, 0.5]]))], np.eye(4)[None], min_points=3, neighbors=1, max_iteration=0).num_correspondences.tolist() == [0]


def test_non_finite_and_range_gated_rows_are_passed_over(ops):
    clouds, poses, _, tables = scene()
    cloud = clouds[4][:2000].copy()
    cloud[5, 0] = np.nan
    cloud[17, 2] = np.inf
    cloud[400, 1] = -np.inf
    lo, hi = 3.0, 20.0
    r = np.linalg.norm(cloud.astype(np.float64), axis=1)
    gated = int(np.sum(np.isfinite(r) & ((r < lo) | (r > hi))))
    assert gated > 100
    res = shared_map(ops, 1.0).register([cuda(cloud)], poses[4:5], max_iteration=0, min_range=lo, max_range=hi)
    e = RR.evaluate(tables[1.0], cloud, poses[4], 0.02, 4, 1, lo, hi)
    assert res.num_points.tolist() == [e['n_points']] == [2000 - 3 - gated]
    assert res.num_correspondences.tolist() == [e['n_corr']]
    assert np.isfinite(res.cost.cpu().numpy()).all() and np.isfinite(res.information.cpu().numpy()).all()


def test_register_counts_the_points_that_integrate_keeps(ops):
    """The 16 special rows of test_voxel_map_gpu (non-finite values, the gate boundaries, the attribute limit, the extent) as one scan
    under three poses and two range gates: the registration's num_points, the `integrated` counter of a fresh plain map and of a
    fresh map with moments, and both restatements' counts are one number, and that number is the literal one."""
    import voxel_map_restatement as VM
    from test_voxel_map import random_pose
    from test_voxel_map_gpu import special_rows
    rows = special_rows()
    far = np.eye(4)
    far[0, 3] = 314572.8 - 50.0
    poses = (np.eye(4), far, random_pose(np.random.default_rng(2), 100.0))
    gates = ((0.0, np.inf), (5.0, 80.0))
    want = iter((10, 8, 9, 7, 10, 8))
    table = MR.build([rows], [np.eye(4)], 0.3, 4)
    against = ops.VoxelMap(0.3, channels=4, capacity=64, moments=True).integrate([cuda(rows)], np.eye(4)[None])
    for X in poses:
        for lo, hi in gates:
            n = next(want)
            assert len(VM.quantise(rows, X, 0.3, 4, lo, hi)[0]) == n and len(RR.world_points(table, rows, X, lo, hi)[0]) == n
            res = against.register([cuda(rows)], X[None], max_iteration=0, min_range=lo, max_range=hi)
            assert res.num_points.tolist() == [n]
            for moments in (False, True):
                fresh = ops.VoxelMap(0.3, channels=4, capacity=64, moments=moments).integrate([cuda(rows)], X[None], lo, hi)
                assert fresh.stats()['integrated'] == n, (moments, lo, hi)


def test_status_converged_and_max_iteration_and_the_map_is_only_read(ops):
    clouds, _, _, _ = scene()
    vmap = shared_map(ops, 1.0)
    before = (vmap._buf.clone(), vmap._mom.clone())
    X = starts()
    res = vmap.register([cuda(clouds[4])] * 2, X)
    assert res.status.tolist() == [1, 1] and 1 <= int(res.iterations.min()) and int(res.iterations.max()) < 30
    two = vmap.register([cuda(clouds[4])] * 2, X, max_iteration=2)
    assert two.status.tolist() == [0, 0] and two.iterations.tolist() == [2, 2]
    import torch
    assert torch.equal(before[0], vmap._buf) and torch.equal(before[1], vmap._mom)
    assert 'converged after' in repr(res) and 'max_iteration after 2 updates' in repr(two)


def test_arguments_are_rejected_by_name(ops):
    import torch
    clouds, poses, _, _ = scene()
    pts = cuda(clouds[4][:100])
    with pytest.raises(ValueError, match='moments=True'):
        ops.VoxelMap(1.0, channels=3, capacity=64).register([pts], poses[4:5])
    vmap = shared_map(ops, 1.0)
    for kw, match in ((dict(sigma=0.0), 'sigma'), (dict(sigma=float('nan')), 'sigma'), (dict(neighbors=3), 'neighbors'),
                      (dict(min_points=0), 'min_points'), (dict(max_iteration=-1), 'max_iteration'), (dict(rot_eps=-1.0), 'rot_eps'),
                      (dict(trans_eps=-1e-3), 'trans_eps'), (dict(min_range=2.0, max_range=1.0), 'min_range')):
        with pytest.raises(ValueError, match=match):
            vmap.register([pts], poses[4:5], **kw)
    with pytest.raises(ValueError, match=r'poses must be \[1, 4, 4\]'):
        vmap.register([pts], poses[:2])
    bad = poses[4:5].copy()
    bad[0, 1, 3] = np.inf
    with pytest.raises(ValueError, match='finite'):
        vmap.register([pts], bad)
    with pytest.raises(ValueError, match='float32 CUDA'):
        vmap.register([pts.cpu()], poses[4:5])
    with pytest.raises(ValueError, match='float32 CUDA'):
        vmap.register([pts.double()], poses[4:5])
    res = vmap.register([], np.zeros((0, 4, 4)))
    assert res.transformations.shape == (0, 4, 4) and res.status.shape == (0,) and repr(res) == 'MapRegistrationResult()'
    packed = vmap.register((pts, torch.tensor([0, 40, 100])), np.stack([poses[4], poses[4]]), max_iteration=0)
    assert packed.num_points.tolist() == [40, 60]


# ---- the raw C-ABI ---------------------------------------------------------------------------------------------------------------

def test_raw_abi_argument_errors_and_an_empty_batch(ops):
    import torch
    from rdmnet_amd import _lib
    L = _lib.lib()
    clouds, poses, _, _ = scene()
    vmap = shared_map(ops, 1.0)
    pts = cuda(clouds[4][:500])
    off = torch.tensor([0, 500], dtype=torch.int64, device='cuda')
    X = torch.from_numpy(poses[4:5].copy()).cuda()
    out = torch.zeros((59,), dtype=torch.float64, device='cuda')
    stats = torch.zeros((4,), dtype=torch.int64, device='cuda')
    need = L.rdm_voxel_map_register_workspace_bytes(1)
    assert need > 0 and L.rdm_voxel_map_register_workspace_bytes(0) > 0 and L.rdm_voxel_map_register_workspace_bytes(-1) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')

    def call(n_scans=1, moments=vmap._mom.data_ptr(), moments_bytes=vmap._mom.numel(), sigma=0.02, min_points=4, neighbors=1, max_iteration=0,
             rot_eps=0.0, trans_eps=0.0, ws_bytes=need, total=500):
        return L.rdm_voxel_map_register(*vmap._head(), moments, moments_bytes, vmap.voxel, pts.data_ptr(), 3, total, off.data_ptr(),
                                        X.data_ptr(), n_scans, 0.0, float('inf'), sigma, min_points, neighbors, max_iteration, rot_eps,
                                        trans_eps, out[0:].data_ptr(), out[16:].data_ptr(), out[52:].data_ptr(), out[58:].data_ptr(),
                                        stats.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())

    assert call(moments=0) == ERR_ARG and b'null moments' in L.rdm_last_error()
    assert call(moments_bytes=vmap._mom.numel() - 1) == ERR_ARG and b'moments block is too small' in L.rdm_last_error()
    assert call(sigma=0.0) == ERR_ARG and call(sigma=-1.0) == ERR_ARG and b'sigma' in L.rdm_last_error()
    assert call(neighbors=0) == ERR_ARG and call(neighbors=6) == ERR_ARG and b'neighbors must be 1 or 7' in L.rdm_last_error()
    assert call(rot_eps=-1e-9) == ERR_ARG and call(trans_eps=-1.0) == ERR_ARG
    assert call(min_points=0) == ERR_ARG and call(min_points=-3) == ERR_ARG and call(max_iteration=-1) == ERR_ARG
    assert call(n_scans=-1) == ERR_ARG and call(total=-1) == ERR_ARG
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and b'workspace too small' in L.rdm_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not stats.any()  # nothing ran
    assert call(n_scans=0) == 0 and call(n_scans=0, ws_bytes=L.rdm_voxel_map_register_workspace_bytes(0)) == 0
    torch.cuda.synchronize()
    assert not out.any() and not stats.any()
    assert call() == 0
    torch.cuda.synchronize()
    want = vmap.register([pts], poses[4:5], max_iteration=0)
    assert torch.equal(out[:16].view(4, 4), want.transformations[0]) and torch.equal(out[16:52].view(6, 6), want.information[0])
    assert stats.tolist() == [0, int(want.num_correspondences[0]), 500, 0]


# ---- recovery --------------------------------------------------------------------------------------------------------------------

def test_recovery_on_the_gpu(ops):
    """From 5 cm / 5 mrad per axis at neighbors 1 and 7, and from 0.3 m / 0.02 rad at neighbors 7, on the 1 m map: the restatement
    lowers both pose errors in each of these cases (checked first), and so does the library."""
    clouds, poses, _, tables = scene()
    vmap = shared_map(ops, 1.0)
    for sigma_t, sigma_r, neighbors in ((0.05, 0.005, 1), (0.05, 0.005, 7), (0.3, 0.02, 7)):
        X = starts((13, 14), sigma_t, sigma_r)
        res = vmap.register([cuda(clouds[4])] * 2, X, neighbors=neighbors)
        T = res.transformations.cpu().numpy()
        for s in range(2):
            want = RR.register(tables[1.0], clouds[4], X[s], neighbors=neighbors)
            before, ref, got = pose_error(X[s], poses[4]), pose_error(want['transform'], poses[4]), pose_error(T[s], poses[4])
            print(f'{sigma_t} m / {sigma_r} rad, neighbors {neighbors}: {before[0] * 100:.2f} cm / {before[1] * 1e3:.2f} mrad -> '
                  f'{got[0] * 100:.2f} cm / {got[1] * 1e3:.2f} mrad (restatement {ref[0] * 100:.2f} cm / {ref[1] * 1e3:.2f} mrad)')
            assert ref[0] < before[0] and ref[1] < before[1]
            assert got[0] < before[0] and got[1] < before[1]


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_trajectory_map_refine_end_to_end(ops, tmp_path):
    """Four frames of the street with pair poses off by 5 cm / 5 mrad: --map-refine adds the `refined` lines and files, and every
    other line and file is that of a run without the flag."""
    from rdmnet_amd import trajectory
    clouds, poses, _, _ = scene()
    frames = [0, 3, 6, 9]
    data, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    rng = np.random.default_rng(31)
    noisy = [poses[0]] + [perturb(poses[k], rng, 0.05, 0.005) for k in range(1, 4)]
    for k, f in enumerate(frames):
        np.save(folder / ('%06d.npy' % f), clouds[k])
    for k in range(3):
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=np.linalg.inv(noisy[k + 1]) @ noisy[k],
                 transform=np.linalg.inv(poses[k + 1]) @ poses[k], information=np.eye(6))

    def run(name, extra):
        out, lines = tmp_path / name, []
        trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                            '--map-voxel', '1.0', '--map-sharpness', *extra]), emit=lines.append)
        return lines, out

    plain, plain_out = run('plain', [])
    lines, out = run('refined', ['--map-refine', '--map-refine-neighbors', '7', '--map-refine-iterations', '20'])
    assert not any('refined' in s for s in plain) and sorted(os.listdir(plain_out)) == ['5_chained.txt', '5_chained_map.npy']
    assert [s for s in lines if ' refined' not in s] == plain
    for name in os.listdir(plain_out):
        assert open(out / name, 'rb').read() == open(plain_out / name, 'rb').read(), name
    assert sorted(os.listdir(out)) == ['5_chained.txt', '5_chained_map.npy', '5_refined.txt', '5_refined_map.npy']
    added = [s for s in lines if ' refined' in s]
    assert [s.split(':')[0] for s in added] == ['seq 5 refined', 'seq 5 refined against the map', 'seq 5 refined map', 'seq 5 refined sharpness']
    assert added[0].startswith('seq 5 refined: r_rmse: ') and added[1].startswith('seq 5 refined against the map: 4 frames, ')
    assert added[1].endswith(' 0 degenerate frames')
    text = open(out / '5_refined.txt').read().splitlines()
    assert len(text) == 4 and all(len(row.split()) == 12 for row in text)
    assert text[0] == open(out / '5_chained.txt').read().splitlines()[0]  # frame 0 keeps its pose
    # the written map is the one built during the refinement: the scans under the refined poses
    refined = np.array([[float(v) for v in row.split()] + [0, 0, 0, 1] for row in text]).reshape(4, 4, 4)
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    again2, vmap, stats = trajectory.refine_against_map(paths, trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0],
                                                        voxel=1.0, neighbors=7, max_iteration=20)
    assert stats['frames'] == 4 and stats['status'].tolist()[0] == -1 and stats['degenerate'] == 0
    assert np.abs(again2 - refined).max() < 1e-8  # (the file holds nine decimals)
    assert added[1] == trajectory.refine_line(5, stats)
    # with --optimize the base variant is `optimized`, and its own lines and files stay those of a run without the flag
    opt_plain, opt_plain_out = run('opt_plain', ['--optimize'])
    opt_lines, opt_out = run('opt_refined', ['--optimize', '--map-refine'])
    assert [s for s in opt_lines if ' refined' not in s] == opt_plain and len([s for s in opt_lines if ' refined' in s]) == 4
    for name in os.listdir(opt_plain_out):
        assert open(opt_out / name, 'rb').read() == open(opt_plain_out / name, 'rb').read(), name
    assert sorted(set(os.listdir(opt_out)) - set(os.listdir(opt_plain_out))) == ['5_refined.txt', '5_refined_map.npy']
    assert added[3] == trajectory.sharpness_line(5, 'refined', 4, vmap.sharpness(4))
    points, counts, _ = vmap.extract(1)
    assert np.array_equal(np.load(out / '5_refined_map.npy'), np.concatenate([points.cpu().numpy(), counts.cpu().numpy()[:, None].astype(np.float32)], 1))
