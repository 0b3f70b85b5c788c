"""GPU: the map-to-map alignment (rdm_voxel_map_align, ops.VoxelMap.align, `trajectory --map-prior-align`) against the NumPy
restatement tests/voxel_align_restatement.py on the two sessions of test_voxel_align: the evaluation alone within the worst-case
summation bound, a set longer than one stride of its threads, a fixed number of updates, bit equality across runs, batch positions,
capacities, integration orders and the three forms of a source, the edge cases, the raw C-ABI's argument errors, recovery of a
perturbed transform with the merged map as the payoff, and one command-line run.

Session A (the target): scans 0, 2, 4, 6 of the street under their true poses at 1 m voxels; session B (the sources): scans 1, 3, 5, 7
under inv(T) pose at 1 m and 0.5 m; scans of 4 000 points."""
import os

import numpy as np
import pytest

import voxel_align_restatement as AR
import voxel_moments_restatement as MR
from test_voxel_align import A_SCANS, B_SCANS, RECOVERY, SOURCE_VOXELS, sessions, starts
from test_voxel_register import perturb, pose_error

pytestmark = pytest.mark.gpu

SIGMA = 0.02
ERR_ARG, ERR_WORKSPACE = -1, -2  # RDM_ERR_ARG, RDM_ERR_WORKSPACE
K_STRIDE = 64 * 256  # kRegGroups * kBlock: the records of a set that its threads take in one step
# The largest entry-wise difference between the library's transform and the restatement's after five updates, measured over the eight
# cases of test_five_updates_agree_with_the_restatement on the first GPU run: 1.8e-15 (rotation entries and metres alike).  Rounding of
# the differently ordered sums and of the differently formed 3 x 3 inverse, carried through five solves.  The asserted bound is 100 times
# that (the margin is for a record within rounding of a cell face that takes the other voxel in one of the two computations), far
# below the cap of 1e-9.
POSE_MEASURED = 1.8e-15
POSE_BOUND = 100.0 * POSE_MEASURED
_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def cuda(cloud):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).cuda()


def gpu_map(ops, voxel, scans, poses, capacity=1 << 16):
    clouds = sessions()[0]
    return ops.VoxelMap(voxel, channels=3, capacity=capacity, moments=True).integrate([cuda(clouds[k]) for k in scans], poses[list(scans)])


def target_map(ops):
    if 'target' not in _cache:
        _cache['target'] = gpu_map(ops, 1.0, A_SCANS, sessions()[1])
    return _cache['target']


def source_map(ops, voxel):
    if ('source', voxel) not in _cache:
        _cache['source', voxel] = gpu_map(ops, voxel, B_SCANS, sessions()[3])
    return _cache['source', voxel]


def outputs(res):
    return (res.transformations, res.information, res.gradient, res.cost, res.iterations, res.num_correspondences, res.num_points, res.status)


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    import torch
    return all(torch.equal(x[rows_a], y[rows_b]) for x, y in zip(outputs(a), outputs(b)))


def within_bound(res, s, e, voxel_a, voxel_b):
    """Every entry of H, g and cost of row s within 2^-52 (n_corr + 64 kappa) A of the restatement's evaluation e -> the largest ratio."""
    kappa = (voxel_a ** 2 + voxel_b ** 2 + SIGMA ** 2) / SIGMA ** 2
    bound = 2.0 ** -52 * (e['n_corr'] + 64.0 * kappa)
    H, g, cost = res.information[s].cpu().numpy(), res.gradient[s].cpu().numpy(), float(res.cost[s])
    ratios = [np.abs(H - e['H']) / (bound * e['abs_H']), np.abs(g - e['g']) / (bound * e['abs_g']),
              np.abs(cost - e['cost']) / (bound * e['abs_cost'])]
    worst = max(float(np.max(r)) for r in ratios)
    assert worst <= 1.0, (s, [float(np.max(r)) for r in ratios])
    assert np.array_equal(H, H.T)
    return worst


# ---- the evaluation alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('source_voxel', SOURCE_VOXELS)
def test_evaluation_is_within_the_summation_bound(ops, source_voxel, neighbors):
    """max_iteration = 0.  Counts exactly; every entry of cost, g and H within 2^-52 (n_corr + 64 kappa) A of the restatement's, A =
    the restatement's sum of the absolute values of that entry's terms, kappa = (voxel_a^2 + voxel_b^2 + sigma^2) / sigma^2:
    register's worst case of a sum of n_corr terms in another order, plus the differently ordered 3 x 3 inverse, with the
    eigenvalue range of the summed covariance.  Measured: the largest ratio to the bound over the four cases is 1.4e-4."""
    _, _, T, _, target, sources = sessions()
    X = np.concatenate([starts(), T[None]])
    res = target_map(ops).align([source_map(ops, source_voxel)] * 3, X, sigma=SIGMA, neighbors=neighbors, max_iteration=0)
    assert res.status.tolist() == [0, 0, 0] and res.iterations.tolist() == [0, 0, 0]
    assert np.array_equal(res.transformations.cpu().numpy(), X)
    worst = 0.0
    for s in range(3):
        e = AR.evaluate(target, sources[source_voxel], X[s], SIGMA, 4, 4, neighbors)
        assert int(res.num_correspondences[s]) == e['n_corr'] and int(res.num_points[s]) == e['n_points']
        assert e['n_corr'] > 1000
        worst = max(worst, within_bound(res, s, e, 1.0, source_voxel))
    print(f'source voxel {source_voxel}, neighbors {neighbors}: largest |difference| / bound = {worst:.3e}')


def test_a_set_longer_than_one_stride_of_its_threads(ops):
    """All eight scans at 0.2 m with source_min_points = 1: more records pass than the 16 384 threads of a set, so a thread's loop
    takes a second step -- the only case here in which it does.  18 736 records, 95 489 pairs; measured ratio to the bound: 1.5e-3."""
    clouds, _, T, in_b, target, _ = sessions()
    table = MR.build(clouds, in_b, 0.2, 3)
    fine = gpu_map(ops, 0.2, range(8), in_b, capacity=1 << 17)
    res = target_map(ops).align([fine], T[None], sigma=SIGMA, source_min_points=1, neighbors=7, max_iteration=0)
    e = AR.evaluate(target, table, T, SIGMA, 4, 1, 7)
    assert int(res.num_points[0]) == e['n_points'] == len(table.keys) > K_STRIDE
    assert int(res.num_correspondences[0]) == e['n_corr'] > K_STRIDE
    worst = within_bound(res, 0, e, 1.0, 0.2)
    print(f'{e["n_points"]} records, {e["n_corr"]} pairs: largest |difference| / bound = {worst:.3e}')


# ---- a fixed number of updates ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('source_voxel', SOURCE_VOXELS)
def test_five_updates_agree_with_the_restatement(ops, source_voxel, neighbors):
    _, _, _, _, target, sources = sessions()
    X = starts()
    res = target_map(ops).align([source_map(ops, source_voxel)] * 2, X, sigma=SIGMA, neighbors=neighbors, max_iteration=5, rot_eps=0.0,
                                trans_eps=0.0)
    assert res.status.tolist() == [0, 0] and res.iterations.tolist() == [5, 5]
    got = res.transformations.cpu().numpy()
    for s in range(2):
        want = AR.align(target, sources[source_voxel], X[s], SIGMA, 4, 4, neighbors, 5, 0.0, 0.0)
        assert want['status'] == 0 and want['iterations'] == 5
        diff = float(np.abs(got[s] - want['transform']).max())
        print(f'source voxel {source_voxel}, neighbors {neighbors}, start {s}: largest transform difference {diff:.3e}')
        assert diff <= POSE_BOUND <= 1e-9
        assert int(res.num_correspondences[s]) == want['n_corr']
        assert got[s, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


# ---- bit equality ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
def test_runs_batch_positions_and_empty_sets_do_not_change_a_bit(ops, neighbors):
    _, _, T, _, _, _ = sessions()
    target, src, half = target_map(ops), source_map(ops, 1.0), source_map(ops, 0.5)
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=neighbors, max_iteration=6)
    alone = target.align([src], X[:1], **kw)
    assert same(alone, target.align([src], X[:1], **kw))
    assert int(alone.iterations[0]) >= 1 and int(alone.num_correspondences[0]) > 1000
    empty = ops.VoxelMap(1.0, channels=3, capacity=64, moments=True)
    batch = [src, empty, src, src, src, empty]
    Xb = np.stack([T, np.eye(4), X[0], X[1], X[0], X[1]])
    both = target.align(batch, Xb, **kw)
    assert same(both, target.align(batch, Xb, **kw))
    assert same(alone, both, rows_b=slice(2, 3)) and same(alone, both, rows_b=slice(4, 5))
    first = target.align([src, src], np.stack([X[0], T]), **kw)
    assert same(alone, first, rows_b=slice(0, 1))
    # an empty set is degenerate where it stands and moves nothing
    assert both.status[[1, 5]].tolist() == [2, 2] and both.num_points[[1, 5]].tolist() == [0, 0]
    assert np.array_equal(both.transformations[[1, 5]].cpu().numpy(), Xb[[1, 5]])
    assert not both.information[[1, 5]].any() and not both.gradient[[1, 5]].any() and not both.cost[[1, 5]].any()
    # the other grid beside it changes nothing either (one call takes one source voxel size: two calls)
    assert same(target.align([half], X[:1], **kw), target.align([half, half], X, **kw), rows_b=slice(0, 1))


def near(cloud, n):
    return cloud[np.argsort(np.linalg.norm(cloud, axis=1), kind='stable')[:n]]


def test_capacity_and_growth_do_not_change_a_bit(ops):
    clouds, poses, _, _, _, _ = sessions()
    part = near(clouds[2], 2000)
    src, X = source_map(ops, 1.0), starts()
    small = ops.VoxelMap(1.0, channels=3, capacity=1 << 12, moments=True).integrate([cuda(part)], poses[2:3])
    assert small.capacity == 1 << 12
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4)
    before = small.align([src, src], X, **kw)
    assert int(before.num_correspondences.min()) > 300
    small._reserve(28000)  # what a batch of 28 000 points would make integrate do
    assert small.capacity == 1 << 16
    assert same(before, small.align([src, src], X, **kw))
    large = ops.VoxelMap(1.0, channels=3, capacity=1 << 16, moments=True).integrate([cuda(part)], poses[2:3])
    assert same(before, large.align([src, src], X, **kw))


def test_the_order_of_integration_of_either_map_does_not_change_a_bit(ops):
    _, poses, _, in_b, _, _ = sessions()
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4)
    a = target_map(ops).align([source_map(ops, 0.5)] * 2, X, **kw)
    b = gpu_map(ops, 1.0, A_SCANS[::-1], poses, capacity=1 << 17).align([gpu_map(ops, 0.5, B_SCANS[::-1], in_b, capacity=1 << 15)] * 2, X, **kw)
    assert same(a, b)


def test_a_source_as_a_map_its_state_and_its_file_are_one_source(ops, tmp_path):
    target, src = target_map(ops), source_map(ops, 0.5)
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4)
    a = target.align([src, src], X, **kw)
    state = src.state()
    path = src.save(str(tmp_path / 'source.npz'))
    assert same(a, target.align([state, state], X, **kw))
    assert same(a, target.align([src, ops.read_state(path)], X, **kw))
    assert same(a, target.align([ops.read_state(path), state], X, **kw))


# ---- edge cases ------------------------------------------------------------------------------------------------------------------

def test_a_source_far_from_the_target_is_degenerate_and_keeps_its_pose(ops):
    T = sessions()[2]
    X = T.copy()
    X[:3, 3] += [1000.0, -2000.0, 50.0]
    src = source_map(ops, 1.0)
    res = target_map(ops).align([src], X[None])
    assert res.status.tolist() == [2] and res.num_correspondences.tolist() == [0] and res.iterations.tolist() == [0]
    assert res.num_points.tolist() == [int((sessions()[5][1.0].map.counts >= 4).sum())]
    assert np.array_equal(res.transformations[0].cpu().numpy(), X)
    assert not res.information.any() and not res.gradient.any() and not res.cost.any()
    assert 'degenerate after 0 updates, 0 correspondences' in repr(res)


def test_both_min_points_boundaries(ops):
    """Voxel (0, 0, 0) of a 1 m map holds three points and voxel (-2, 1, 0) four; the map is aligned to itself at the identity with
    the own cell alone.  source_min_points 3, 4, 5 let two, one and no record pass (a record that does not is counted nowhere);
    min_points 3, 4, 5 let two, one and none of the two records that pass find its voxel."""
    rng = np.random.default_rng(8)
    cloud = np.concatenate([rng.uniform(0.2, 0.8, (3, 3)), rng.uniform(0.2, 0.8, (4, 3)) + [-2.0, 1.0, 0.0]]).astype(np.float32)
    vmap = ops.VoxelMap(1.0, channels=3, capacity=64, moments=True).integrate([cuda(cloud)], np.eye(4)[None])
    table = MR.build([cloud], [np.eye(4)], 1.0, 3)
    for least, want in ((3, 2), (4, 1), (5, 0)):
        res = vmap.align([vmap], np.eye(4)[None], min_points=1, source_min_points=least, neighbors=1, max_iteration=0)
        e = AR.evaluate(table, table, np.eye(4), 0.02, 1, least, 1)
        assert res.num_correspondences.tolist() == [want] == [e['n_corr']] and res.num_points.tolist() == [want] == [e['n_points']]
        res = vmap.align([vmap], np.eye(4)[None], min_points=least, source_min_points=1, neighbors=1, max_iteration=0)
        e = AR.evaluate(table, table, np.eye(4), 0.02, least, 1, 1)
        assert res.num_correspondences.tolist() == [want] == [e['n_corr']] and res.num_points.tolist() == [2] == [e['n_points']]
        assert not res.gradient.any() and not res.cost.any()  # every residual is exactly zero


def test_single_point_voxels_have_a_zero_covariance_and_finite_outputs(ops):
    clouds, _, T, in_b, target, _ = sessions()
    dust = gpu_map(ops, 0.01, (1,), in_b, capacity=1 << 14)
    table = MR.build([clouds[1]], in_b[1:2], 0.01, 3)
    assert (table.map.counts == 1).all()
    res = target_map(ops).align([dust], T[None], sigma=SIGMA, source_min_points=1, neighbors=1, max_iteration=3, rot_eps=0.0, trans_eps=0.0)
    e = AR.evaluate(target, table, T, SIGMA, 4, 1, 1)
    assert int(res.num_points[0]) == len(table.keys) and e['n_corr'] > 1000
    for t in outputs(res)[:4]:
        assert np.isfinite(t.cpu().numpy()).all()
    assert res.status.tolist() == [0] and res.iterations.tolist() == [3]
    assert target_map(ops).align([dust], T[None], sigma=SIGMA, neighbors=1, max_iteration=0).num_points.tolist() == [0]  # (none holds 4)


def test_statuses_and_both_maps_are_only_read(ops):
    import torch
    target, src = target_map(ops), source_map(ops, 1.0)
    before = (target._buf.clone(), target._mom.clone(), src._buf.clone(), src._mom.clone())
    X = starts()
    res = target.align([src, src], X)
    assert res.status.tolist() == [1, 1] and 1 <= int(res.iterations.min()) and int(res.iterations.max()) < 30
    two = target.align([src, src], X, max_iteration=2)
    assert two.status.tolist() == [0, 0] and two.iterations.tolist() == [2, 2]
    for a, b in zip(before, (target._buf, target._mom, src._buf, src._mom)):
        assert torch.equal(a, b)
    assert 'converged after' in repr(res) and 'max_iteration after 2 updates' in repr(two)


def test_arguments_are_rejected_by_name(ops):
    T = sessions()[2]
    target, src, half = target_map(ops), source_map(ops, 1.0), source_map(ops, 0.5)
    with pytest.raises(ValueError, match='moments=True'):
        ops.VoxelMap(1.0, channels=3, capacity=64).align([src], T[None])
    with pytest.raises(ValueError, match=r'sources\[1\] needs a map created with moments=True'):
        target.align([src, ops.VoxelMap(1.0, channels=3, capacity=64)], np.stack([T, T]))
    with pytest.raises(ValueError, match=r'sources\[1\]: voxel differs \(0.5 against 1.0\)'):
        target.align([src, half], np.stack([T, T]))
    with pytest.raises(ValueError, match=r'sources\[1\]: voxel differs \(1.0 against 0.5\)'):
        target.align([half.state(), src], np.stack([T, T]))
    state = src.state()
    with pytest.raises(ValueError, match=r'sources\[0\] holds no moments'):
        target.align([{k: v for k, v in state.items() if k != 'moments'}], T[None])
    with pytest.raises(ValueError, match=r'sources\[0\]: counts must be'):
        target.align([dict(state, counts=state['counts'].long())], T[None])
    with pytest.raises(ValueError, match=r'sources\[0\] must be a VoxelMap or a state dict'):
        target.align([T], T[None])
    with pytest.raises(ValueError, match='sources must be a list'):
        target.align(src, T[None])
    for kw, match in ((dict(sigma=0.0), 'sigma'), (dict(sigma=float('nan')), 'sigma'), (dict(neighbors=3), 'neighbors'),
                      (dict(min_points=0), 'min_points'), (dict(source_min_points=0), 'source_min_points'),
                      (dict(max_iteration=-1), 'max_iteration'), (dict(rot_eps=-1.0), 'rot_eps'), (dict(trans_eps=-1e-3), 'trans_eps')):
        with pytest.raises(ValueError, match=match):
            target.align([src], T[None], **kw)
    with pytest.raises(ValueError, match=r'poses must be \[1, 4, 4\]'):
        target.align([src], np.stack([T, T]))
    bad = T[None].copy()
    bad[0, 1, 3] = np.inf
    with pytest.raises(ValueError, match='finite'):
        target.align([src], bad)
    res = target.align([], np.zeros((0, 4, 4)))
    assert res.transformations.shape == (0, 4, 4) and res.status.shape == (0,) and repr(res) == 'MapRegistrationResult()'


# ---- the raw C-ABI ---------------------------------------------------------------------------------------------------------------

def test_raw_abi_argument_errors_and_an_empty_batch(ops):
    import torch
    from rdmnet_amd import _lib
    L = _lib.lib()
    T = sessions()[2]
    target, src = target_map(ops), source_map(ops, 0.5)
    st = src.state()
    total = int(st['counts'].shape[0])
    counts, sums, moments = st['counts'].contiguous(), st['sums'].contiguous(), st['moments'].contiguous()
    off = torch.tensor([0, total], dtype=torch.int64, device='cuda')
    X = torch.from_numpy(T[None].copy()).cuda()
    out = torch.zeros((59,), dtype=torch.float64, device='cuda')
    stats = torch.zeros((4,), dtype=torch.int64, device='cuda')
    need = L.rdm_voxel_map_align_workspace_bytes(1)
    assert need > 0 and L.rdm_voxel_map_align_workspace_bytes(0) > 0 and L.rdm_voxel_map_align_workspace_bytes(-1) == 0
    assert need == L.rdm_voxel_map_register_workspace_bytes(1)  # the same carve
    ws = torch.empty((need,), dtype=torch.uint8, device='cuda')

    def call(n_sets=1, moments_block=target._mom.data_ptr(), moments_bytes=target._mom.numel(), voxel=target.voxel, counts_ptr=counts.data_ptr(),
             sums_ptr=sums.data_ptr(), sums_ld=3, moment_sums=moments.data_ptr(), source_voxel=0.5, total=total, sigma=0.02, min_points=4,
             source_min_points=4, neighbors=1, max_iteration=0, rot_eps=0.0, trans_eps=0.0, ws_bytes=need):
        return L.rdm_voxel_map_align(*target._head(), moments_block, moments_bytes, voxel, counts_ptr, sums_ptr, sums_ld, moment_sums,
                                     source_voxel, total, off.data_ptr(), X.data_ptr(), n_sets, sigma, min_points, source_min_points,
                                     neighbors, max_iteration, rot_eps, trans_eps, out[0:].data_ptr(), out[16:].data_ptr(),
                                     out[52:].data_ptr(), out[58:].data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())

    assert call(moments_block=0) == ERR_ARG and b'null moments' in L.rdm_last_error()
    assert call(moments_bytes=target._mom.numel() - 1) == ERR_ARG and b'moments block is too small' in L.rdm_last_error()
    assert call(counts_ptr=0) == ERR_ARG and b'null counts' in L.rdm_last_error()
    assert call(sums_ptr=0) == ERR_ARG and b'null sums' in L.rdm_last_error()
    assert call(moment_sums=0) == ERR_ARG and b'null moment_sums' in L.rdm_last_error()
    assert call(sums_ld=2) == ERR_ARG and b'sums_ld' in L.rdm_last_error()
    assert call(source_voxel=0.0) == ERR_ARG and call(source_voxel=float('inf')) == ERR_ARG and b'source_voxel' in L.rdm_last_error()
    assert call(voxel=-1.0) == ERR_ARG and b'voxel must be positive' in L.rdm_last_error()
    assert call(sigma=0.0) == ERR_ARG and call(sigma=-1.0) == ERR_ARG and b'sigma' in L.rdm_last_error()
    assert call(neighbors=0) == ERR_ARG and call(neighbors=6) == ERR_ARG and b'neighbors must be 1 or 7' in L.rdm_last_error()
    assert call(rot_eps=-1e-9) == ERR_ARG and call(trans_eps=-1.0) == ERR_ARG and b'trans_eps' in L.rdm_last_error()
    assert call(min_points=0) == ERR_ARG and call(source_min_points=0) == ERR_ARG and b'source_min_points' in L.rdm_last_error()
    assert call(max_iteration=-1) == ERR_ARG
    assert call(n_sets=-1) == ERR_ARG and call(n_sets=(1 << 20) + 1) == ERR_ARG and call(total=-1) == ERR_ARG and b'n_sets' in L.rdm_last_error()
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and b'workspace too small' in L.rdm_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not stats.any()  # nothing ran
    assert call(n_sets=0) == 0 and call(n_sets=0, ws_bytes=L.rdm_voxel_map_align_workspace_bytes(0)) == 0
    assert call(total=0, counts_ptr=0, sums_ptr=0, moment_sums=0, n_sets=0) == 0
    torch.cuda.synchronize()
    assert not out.any() and not stats.any()
    assert call() == 0
    torch.cuda.synchronize()
    want = target.align([src], T[None], neighbors=1, max_iteration=0)
    assert torch.equal(out[:16].view(4, 4), want.transformations[0]) and torch.equal(out[16:52].view(6, 6), want.information[0])
    assert torch.equal(out[52:58], want.gradient[0]) and torch.equal(out[58:], want.cost)
    assert stats.tolist() == [0, int(want.num_correspondences[0]), int(want.num_points[0]), 0] and stats[1] > 1000
    # a state's [M, C] sums are passed as they are: only the first three columns are read
    wide = torch.cat([sums, torch.full((total, 2), 1 << 40, dtype=torch.int64, device='cuda')], 1).contiguous()
    first = out.clone()
    assert call(sums_ptr=wide.data_ptr(), sums_ld=5) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ---- recovery --------------------------------------------------------------------------------------------------------------------

def test_recovery_on_the_gpu_and_the_merged_map(ops):
    """From 5 cm / 5 mrad per axis at neighbors 1 and 7, and from 0.3 m / 0.02 rad at neighbors 7, for both source sizes: the
    restatement lowers both errors in each of these cases (checked first), and so does the library.  The payoff without ground truth:
    session B rebuilt under T_aligned pose and merged into A has fewer voxels (at 0.3 m) than the same merge under the start."""
    clouds, poses, T, in_b, target, sources = sessions()
    gpu_target = target_map(ops)
    for source_voxel in SOURCE_VOXELS:
        for sigma_t, sigma_r, neighbors in RECOVERY:
            X = starts((13, 14), sigma_t, sigma_r)
            res = gpu_target.align([source_map(ops, source_voxel)] * 2, X, neighbors=neighbors)
            got_T = res.transformations.cpu().numpy()
            for s in range(2):
                want = AR.align(target, sources[source_voxel], X[s], neighbors=neighbors)
                before, ref, got = pose_error(X[s], T), pose_error(want['transform'], T), pose_error(got_T[s], T)
                print(f'source voxel {source_voxel}, {sigma_t} m / {sigma_r} rad, neighbors {neighbors}: {before[0] * 100:.2f} cm / '
                      f'{before[1] * 1e3:.2f} mrad -> {got[0] * 100:.2f} cm / {got[1] * 1e3:.2f} mrad (restatement {ref[0] * 100:.2f} cm / '
                      f'{ref[1] * 1e3:.2f} mrad)')
                assert ref[0] < before[0] and ref[1] < before[1]
                assert got[0] < before[0] and got[1] < before[1]
    start = starts((13,), 0.3, 0.02)
    aligned = gpu_target.align([source_map(ops, 1.0)], start, neighbors=7).transformations[0].cpu().numpy()

    def merged(X):
        a = gpu_map(ops, 0.3, A_SCANS, poses, capacity=1 << 17)
        return len(a.merge(gpu_map(ops, 0.3, B_SCANS, X @ in_b, capacity=1 << 17)))

    voxels_aligned, voxels_start = merged(aligned), merged(start[0])
    print(f'merged map at 0.3 m: {voxels_aligned} voxels under the alignment, {voxels_start} under the start')
    assert voxels_aligned < voxels_start


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_trajectory_map_prior_align_end_to_end(ops, tmp_path):
    """Session B's four frames as a sequence whose trajectory starts at the identity of its own first frame, with pair poses off by
    5 cm / 5 mrad; the prior is session A's map in A's frame, so prior <- trajectory is the true pose of B's first scan.
    --map-prior-align adds the `aligned to the prior map` line and {seq}_prior_alignment.txt, and nothing that does not touch the prior
    changes: every line and file of the chained variant is that of a run without the flag whose prior already is in the
    trajectory's frame.  The `localized` variant exists in both runs but is asked of two different priors (the same scans quantised
    on two grids), so its lines and files agree in name and form, not in every digit; it is compared with the truth instead."""
    from rdmnet_amd import trajectory
    clouds, poses, _, _, target, _ = sessions()
    to_prior = poses[B_SCANS[0]]  # prior <- trajectory
    truth = np.linalg.inv(to_prior) @ poses[list(B_SCANS)]
    frames = [0, 3, 6, 9]
    data, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    rng = np.random.default_rng(31)
    noisy = [truth[0]] + [perturb(truth[k], rng, 0.05, 0.005) for k in range(1, 4)]
    for k, f in enumerate(frames):
        np.save(folder / ('%06d.npy' % f), clouds[B_SCANS[k]])
    for k in range(3):
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=np.linalg.inv(noisy[k + 1]) @ noisy[k],
                 transform=np.linalg.inv(truth[k + 1]) @ truth[k], information=np.eye(6))
    prior_a = target_map(ops).save(str(tmp_path / 'prior.npz'))
    moved = tmp_path / 'moved'
    moved.mkdir()
    prior_b = gpu_map(ops, 1.0, A_SCANS, np.linalg.inv(to_prior) @ poses).save(str(moved / 'prior.npz'))  # A's map in the trajectory's frame
    initial = str(tmp_path / 'initial.txt')
    start = perturb(to_prior, np.random.default_rng(32), 0.05, 0.005)
    np.savetxt(initial, start[:3], fmt='%.17e')

    def run(name, extra):
        out, lines = tmp_path / name, []
        trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                            '--map-voxel', '1.0', '--map-refine-neighbors', '7', '--map-localize',
                                                            *extra]), emit=lines.append)
        return lines, out

    plain, plain_out = run('plain', ['--map-prior', prior_b])
    lines, out = run('aligned', ['--map-prior', prior_a, '--map-prior-align', '--map-prior-initial', initial])
    blind, blind_out = run('blind', ['--map-prior', prior_a])
    added = [s for s in lines if 'aligned to the prior map' in s]
    assert len(added) == 1 and added[0].startswith('seq 5 chained aligned to the prior map prior.npz: ') and added[0].endswith('(converged)')
    assert lines.index(added[0]) == 2 and lines[1].startswith('seq 5 chained map: ')  # after the base variant's map lines
    rest = [s for s in lines if s != added[0]]
    assert [s.split()[:3] for s in rest] == [s.split()[:3] for s in plain]  # (the same lines, of the same variants)
    assert [s for s in rest if ' localized' not in s] == [s for s in plain if ' localized' not in s]
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain_out))) == ['5_prior_alignment.txt'] and set(os.listdir(plain_out)) <= set(os.listdir(out))
    for name in os.listdir(plain_out):
        if 'localized' not in name:
            assert open(out / name, 'rb').read() == open(plain_out / name, 'rb').read(), name
    # the file: the restatement's alignment of the chained map, through nine decimals
    text = open(out / '5_prior_alignment.txt').read().splitlines()
    assert len(text) == 4 and all(len(row.split()) == 4 for row in text)
    written = np.array([[float(v) for v in row.split()] for row in text])
    chained = trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0]
    want = AR.align(target, MR.build([clouds[k] for k in B_SCANS], chained, 1.0, 3), trajectory.read_transform(initial), 0.02, 4, 4, 7, 30)
    assert want['status'] == 1
    assert np.abs(written - want['transform']).max() < 1e-8 and POSE_BOUND <= 1e-9
    assert written[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    before, after = pose_error(start, to_prior), pose_error(written, to_prior)
    print(f'prior <- trajectory: {before[0] * 100:.2f} cm / {before[1] * 1e3:.2f} mrad -> {after[0] * 100:.2f} cm / {after[1] * 1e3:.2f} mrad')
    assert after[0] < before[0] and after[1] < before[1]
    # from Python: the same transform and the same line
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    again, stats = trajectory.align_to_map(paths, chained, ops.VoxelMap.load(prior_a), trajectory.read_transform(initial), voxel=1.0, neighbors=7)
    assert np.abs(again - written).max() < 1e-8 and stats['status'] == 1 and stats['voxels'] >= stats['matched'] > 0
    assert added[0] == trajectory.align_line(5, 'chained', dict(name='prior.npz'), stats)

    # the localized poses stay in the trajectory's frame and are closer to the truth than with the unaligned prior
    def error(folder_out):
        rows = np.loadtxt(folder_out / '5_localized.txt').reshape(4, 3, 4)
        return float(np.mean([np.linalg.norm(rows[k, :, 3] - truth[k, :3, 3]) for k in range(4)]))

    print(f'mean translation error of `localized`: {error(out) * 100:.2f} cm aligned, {error(blind_out) * 100:.2f} cm unaligned, '
          f'{error(plain_out) * 100:.2f} cm with the prior in the trajectory frame')
    assert error(out) < error(blind_out)
    assert not any('aligned to the prior map' in s for s in plain + blind)
    with pytest.raises(trajectory.TrajectoryError, match='--map-prior-initial needs --map-prior-align'):
        run('refused', ['--map-prior', prior_a, '--map-prior-initial', initial])
    # with --optimize the base variant is `optimized`: its map is the one aligned, and the line follows its map lines
    opt_plain, _ = run('opt_plain', ['--optimize', '--map-prior', prior_b])
    opt_lines, opt_out = run('opt_aligned', ['--optimize', '--map-prior', prior_a, '--map-prior-align', '--map-prior-initial', initial])
    opt_added = [s for s in opt_lines if 'aligned to the prior map' in s]
    assert len(opt_added) == 1 and opt_added[0].startswith('seq 5 optimized aligned to the prior map prior.npz: ')
    assert opt_lines[opt_lines.index(opt_added[0]) - 1].startswith('seq 5 optimized map: ')
    assert [s for s in opt_lines if ' localized' not in s and s != opt_added[0]] == [s for s in opt_plain if ' localized' not in s]
    assert os.path.isfile(opt_out / '5_prior_alignment.txt')
    # a start outside the basin ends in a TrajectoryError that names the sequence
    np.savetxt(initial, np.eye(4)[:3] + [[0, 0, 0, 1000.0], [0, 0, 0, 0], [0, 0, 0, 0]])
    with pytest.raises(trajectory.TrajectoryError, match='seq 5: the alignment of the chained map to the prior map prior.npz is degenerate'):
        run('degenerate', ['--map-prior', prior_a, '--map-prior-align', '--map-prior-initial', initial])
