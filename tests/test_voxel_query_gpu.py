"""GPU: the per-point queries of the voxel map (rdm_voxel_map_query, ops.VoxelMap.query and .clean, `trajectory --map-clean`) against
the NumPy restatement tests/voxel_query_restatement.py: on the street with the moving car of test_voxel_query (against the map of all
eight scans, with moments and observations, and against the map of the street alone) and on the six scans of test_voxel_observations_gpu.fixture (far from the origin, under any
rotation), at 0.3 m and 1 m voxels and neighbors 1 and 7.  The integer outputs are compared with np.array_equal, the two distances per
row within 2^-52 (1 + 64 kappa) A, A = the restatement's sum of the absolute values of the row's terms r_a M_ab r_b and kappa =
(voxel^2 + sigma^2) / sigma^2 for the differently ordered 3 x 3 inverse (test_voxel_register_gpu's term).  So that an integer cannot
hide a near tie, `reference` asserts on the restatement, before the GPU is asked, that no row's d2 lies within that bound of max_d2
and that no row's two smallest d2_o lie within it of each other: no row is excused."""
import itertools
import os

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_observations_restatement as OR
import voxel_query_restatement as QR
import voxel_register_restatement as RR
from test_voxel_map_gpu import dev, special_rows
from test_voxel_observations_gpu import fixture as six_scans
from test_voxel_query import CAR, scene

pytestmark = pytest.mark.gpu

VOXELS = (0.3, 1.0)
SIGMA = 0.02
MAX_D2 = 25.0
ERR_ARG, ERR_WORKSPACE = -1, -2  # RDM_ERR_ARG, RDM_ERR_WORKSPACE
FIELDS = ('labels', 'best', 'counts', 'scans', 'first', 'last', 'd2', 'd2_sum', 'pairs', 'tallies')
_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def kappa(voxel, sigma=SIGMA):
    return (voxel ** 2 + sigma ** 2) / sigma ** 2


def bound_of(voxel, A, sigma=SIGMA):
    return 2.0 ** -52 * (1.0 + 64.0 * kappa(voxel, sigma)) * A


def data(name, scans):
    """-> (the scans that are queried, poses, channels): `street` and `prior` = the eight scans with the car, `six` = the six
    nearest-300 scans."""
    if name in ('street', 'prior'):
        _, _, clouds, poses = scene(5)
        return clouds, poses, 3
    clouds, poses, _ = six_scans(scans)
    return clouds, poses, 4


def mapped(name, scans):
    """The scans that the map holds: the queried ones, but for `prior` the street without the car."""
    return scene(5)[0] if name == 'prior' else data(name, scans)[0]


def reference(name, scans, voxel, neighbors):
    """The restatement's maps of the scans and its answers for the same scans (min_scans 2, MAX_D2), after the assertion that no
    row is near a tie; computed once, never changed."""
    key = (name, voxel, neighbors)
    if key not in _cache:
        clouds, poses, C = data(name, scans)
        if ('maps', name, voxel) not in _cache:
            _cache['maps', name, voxel] = (MR.build(mapped(name, scans), poses, voxel, C), OR.build(mapped(name, scans), poses, voxel, C))
        table, observed = _cache['maps', name, voxel]
        ref = QR.batch(table, observed, clouds, poses, sigma=SIGMA, min_points=1, neighbors=neighbors, min_scans=2, max_d2=MAX_D2)
        has = ref['best'] >= 0
        want = {QR.TRANSIENT, QR.STATIC} | ({QR.OFF_SURFACE} if name == 'prior' and voxel == 1.0 else set())
        assert has.sum() > 1000 and want <= set(ref['labels'].tolist())
        assert (np.abs(ref['d2'][has] - MAX_D2) > bound_of(voxel, ref['abs_d2'][has])).all(), 'a d2 within the bound of max_d2'
        two = np.sort(ref['each'], 1)[:, :2]
        rival = np.isfinite(two[:, 1])
        assert neighbors == 1 or rival.sum() > 100
        assert (two[rival, 1] - two[rival, 0] > 2.0 * bound_of(voxel, ref['abs_sum'][rival])).all(), 'two voxels within the bound of each other'
        _cache[key] = ref
    return _cache[key]


def gpu_map(ops, name, scans, voxel, capacity=1 << 16, moments=True, observations=True, order=None):
    (_, poses, C), clouds = data(name, scans), mapped(name, scans)
    order = list(range(len(clouds))) if order is None else order
    return ops.VoxelMap(voxel, channels=C, capacity=capacity, moments=moments, observations=observations).integrate(
        [dev(clouds[k]) for k in order], poses[order])


def shared_map(ops, name, scans, voxel):
    if ('gpu', name, voxel) not in _cache:
        _cache['gpu', name, voxel] = gpu_map(ops, name, scans, voxel)
    return _cache['gpu', name, voxel]


def fields(res, names=FIELDS):
    return [getattr(res, k) for k in names]


def same(a, b, rows_a=slice(None), rows_b=slice(None), names=FIELDS[:-1]):
    import torch
    return all(torch.equal(x[rows_a], y[rows_b]) for x, y in zip(fields(a, names), fields(b, names)))


def compare(res, ref, voxel, sigma=SIGMA, what=''):
    """-> the largest ratio of a distance's difference to its bound."""
    for k in QR.INTEGERS + ('tallies',):
        got = getattr(res, k).cpu().numpy()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, (what, k, got.dtype, got.shape)
        assert np.array_equal(got, ref[k]), f'{what} {k}: {int((got != ref[k]).sum())} of {got.size} values differ'
    worst = 0.0
    for k, A in (('d2', 'abs_d2'), ('d2_sum', 'abs_sum')):
        got = getattr(res, k).cpu().numpy()
        finite = np.isfinite(ref[k])
        assert np.array_equal(got[~finite], ref[k][~finite])  # +inf where there is no voxel
        nz = finite & (ref[A] > 0)
        assert np.array_equal(got[finite & ~nz], ref[k][finite & ~nz])
        ratio = np.abs(got[nz] - ref[k][nz]) / bound_of(voxel, ref[A][nz], sigma)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (ratio <= 1.0).all(), (what, k, float(ratio.max()))
    return worst


# ---- against the restatement ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
@pytest.mark.parametrize('name', ('street', 'six', 'prior'))
def test_every_output_against_the_restatement(ops, scans, name, voxel, neighbors):
    """`prior`: the street's scans with the car against the map of the street alone, where points are unmapped and off the surface too.
    Measured: the largest |difference| / bound over the twelve cases is 1.5e-3."""
    import torch
    ref = reference(name, scans, voxel, neighbors)
    clouds, poses, _ = data(name, scans)
    res = shared_map(ops, name, scans, voxel).query([dev(c) for c in clouds], poses, sigma=SIGMA, neighbors=neighbors, min_scans=2,
                                                    max_d2=MAX_D2)
    assert res.LABELS == QR.LABELS and torch.equal(res.offsets.cpu(), torch.from_numpy(ref['offsets']))
    worst = compare(res, ref, voxel, what=f'{name} {voxel} {neighbors}')
    print(f'{name}, voxel {voxel}, neighbors {neighbors}: tallies {ref["tallies"].sum(0).tolist()}, largest |difference| / bound = {worst:.3e}')
    if name == 'street' and voxel == 0.3:  # what the feature is for: every point of the car is transient
        is_car = np.concatenate([np.arange(len(c)) >= len(c) - CAR for c in clouds])
        assert (res.labels.cpu().numpy()[is_car] == QR.TRANSIENT).all()


@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
def test_agreement_with_the_registration(ops, scans, voxel, neighbors):
    """The sum of a scan's d2_sum against register(max_iteration=0).cost: the terms are the same bits (one piece of code forms them), so
    the two differ by the order of two sums of n_corr terms -- inside the evaluation's bound 2^-52 (n_corr + 64 kappa) A of
    test_voxel_register_gpu; pairs and labels against its two counts exactly."""
    clouds, poses, _ = data('street', scans)
    vmap = shared_map(ops, 'street', scans, voxel)
    table = reference('street', scans, voxel, neighbors) and _cache['maps', 'street', voxel][0]
    X = np.stack([RR.apply(X, np.array([0.001, -0.002, 0.001, 0.02, -0.01, 0.01])) for X in poses])
    pts = [dev(c) for c in clouds]
    res = vmap.query(pts, X, sigma=SIGMA, min_points=4, neighbors=neighbors)
    reg = vmap.register(pts, X, sigma=SIGMA, min_points=4, neighbors=neighbors, max_iteration=0)
    off = res.offsets.tolist()
    assert res.tallies[:, 7].tolist() == reg.num_correspondences.tolist() and min(reg.num_correspondences.tolist()) > 300
    assert res.tallies[:, 3:7].sum(1).tolist() == reg.num_points.tolist() == [len(c) for c in clouds]
    for s in range(len(clouds)):
        e = RR.evaluate(table, clouds[s], X[s], SIGMA, 4, neighbors)
        got, want = float(res.d2_sum[off[s]:off[s + 1]].sum()), float(reg.cost[s])
        assert abs(got - want) <= 2.0 ** -52 * (e['n_corr'] + 64.0 * kappa(voxel)) * e['abs_cost'], (s, got, want)


# ---- invariance, bit for bit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
def test_runs_batch_positions_an_empty_scan_and_the_packed_form_do_not_change_a_bit(ops, scans, neighbors):
    import torch
    clouds, poses, _ = data('six', scans)
    vmap = shared_map(ops, 'six', scans, 0.3)
    kw = dict(sigma=SIGMA, neighbors=neighbors, min_scans=2, max_d2=MAX_D2)
    alone = vmap.query([dev(clouds[2])], poses[2:3], **kw)
    assert same(alone, vmap.query([dev(clouds[2])], poses[2:3], **kw)) and torch.equal(alone.tallies, vmap.query([dev(clouds[2])], poses[2:3], **kw).tallies)
    tiny = [(k % 6, clouds[k % 6][3 * k:3 * k + 17]) for k in range(69)]  # 69 tiny scans: with the scan, 70 > 64 scans in one call
    batch = [dev(c) for _, c in tiny[:35]] + [dev(clouds[2]), dev(clouds[0][:0])] + [dev(c) for _, c in tiny[35:]]
    X = np.concatenate([poses[[k for k, _ in tiny[:35]]], poses[2:3], poses[:1], poses[[k for k, _ in tiny[35:]]]])
    res = vmap.query(batch, X, **kw)
    lo = 35 * 17
    assert len(batch) == 71 and same(alone, res, rows_b=slice(lo, lo + len(clouds[2])))
    assert torch.equal(res.tallies[35], alone.tallies[0]) and res.tallies[36].tolist() == [0] * 8
    for k in (0, 34, 37, 70):
        one = vmap.query([batch[k]], X[k:k + 1], **kw)
        assert torch.equal(res.tallies[k], one.tallies[0]) and same(one, res, rows_b=slice(int(res.offsets[k]), int(res.offsets[k + 1])))
    packed = vmap.query((torch.cat(batch), res.offsets.cpu()), X, **kw)
    assert same(res, packed, names=FIELDS)
    wide = torch.zeros((len(clouds[2]), 7), device='cuda')  # ld > channels
    wide[:, :4] = dev(clouds[2])
    assert same(alone, vmap.query([wide], poses[2:3], **kw), names=FIELDS)
    assert same(alone, vmap.query((wide, torch.tensor([0, len(wide)])), poses[2:3], **kw), names=FIELDS)


@pytest.mark.parametrize('neighbors', (1, 7))
def test_capacity_growth_and_the_order_of_integration_do_not_change_a_bit(ops, scans, neighbors):
    clouds, poses, _ = data('six', scans)
    pts = [dev(c) for c in clouds]
    kw = dict(sigma=SIGMA, neighbors=neighbors, min_scans=2, max_d2=MAX_D2)
    want = shared_map(ops, 'six', scans, 0.3).query(pts, poses, **kw)
    small, grown = gpu_map(ops, 'six', scans, 0.3, capacity=4096), gpu_map(ops, 'six', scans, 0.3, capacity=64)
    assert small.capacity < 1 << 16 and grown.capacity > 64
    assert same(want, small.query(pts, poses, **kw), names=FIELDS) and same(want, grown.query(pts, poses, **kw), names=FIELDS)
    # the rows of every scan shuffled: other slots, other arrival orders, the same scan ids
    rng = np.random.default_rng(3)
    shuffled = ops.VoxelMap(0.3, channels=4, capacity=1 << 16, moments=True, observations=True).integrate(
        [dev(c[rng.permutation(len(c))]) for c in clouds], poses)
    assert same(want, shuffled.query(pts, poses, **kw), names=FIELDS)
    # the scans in reverse (their ids change with it: a map without observations)
    names = tuple(k for k in FIELDS if k not in ('scans', 'first', 'last'))
    kw['min_scans'] = 1
    a = gpu_map(ops, 'six', scans, 0.3, observations=False).query(pts, poses, **kw)
    b = gpu_map(ops, 'six', scans, 0.3, observations=False, order=[5, 4, 3, 2, 1, 0]).query(pts, poses, **kw)
    assert a.scans is None and same(a, b, names=names)


# ---- null handling -----------------------------------------------------------------------------------------------------------------

def test_every_subset_of_the_outputs_is_the_full_call(ops, scans):
    import torch
    clouds, poses, _ = data('six', scans)
    vmap = shared_map(ops, 'six', scans, 1.0)
    pts = [dev(clouds[1]), dev(clouds[4])]
    for neighbors, max_d2 in ((1, MAX_D2), (1, np.inf), (7, np.inf)):
        kw = dict(sigma=SIGMA, neighbors=neighbors, min_scans=2, max_d2=max_d2)
        full = vmap.query(pts, poses[[1, 4]], **kw)
        assert all(t is not None for t in fields(full))
        sizes = (1, 2, 9) if neighbors == 7 or max_d2 == MAX_D2 else range(11)  # the lookup-only kernel: all 1024 subsets
        for r in sizes:
            for names in itertools.combinations(FIELDS, r):
                res = vmap.query(pts, poses[[1, 4]], outputs=names, **kw)
                for k in FIELDS:
                    got = getattr(res, k)
                    assert (got is None) == (k not in names) and (got is None or torch.equal(got, getattr(full, k))), (names, k)


def test_a_map_without_moments_and_a_map_without_observations(ops, scans):
    clouds, poses, _ = data('six', scans)
    pts = [dev(c) for c in clouds]
    table, observed = reference('six', scans, 1.0, 7) and _cache['maps', 'six', 1.0]
    sigma = 0.1  # d2 = |r|^2 / sigma^2: a sigma at which MAX_D2 is among the distances
    ref = QR.batch(table, observed, clouds, poses, sigma=sigma, neighbors=7, min_scans=2, max_d2=MAX_D2, moments=False)
    has = ref['best'] >= 0
    assert {QR.OFF_SURFACE, QR.STATIC} <= set(ref['labels'].tolist())
    assert (np.abs(ref['d2'][has] - MAX_D2) > bound_of(0.0, ref['abs_d2'][has], sigma)).all()
    two = np.sort(ref['each'], 1)[:, :2]
    rival = np.isfinite(two[:, 1])
    assert (two[rival, 1] - two[rival, 0] > 2.0 * bound_of(0.0, ref['abs_sum'][rival], sigma)).all()
    flat = gpu_map(ops, 'six', scans, 1.0, moments=False)
    worst = compare(flat.query(pts, poses, sigma=sigma, neighbors=7, min_scans=2, max_d2=MAX_D2), ref, 0.0, sigma, 'no moments')
    print(f'no moments: largest |difference| / bound = {worst:.3e} (kappa = 1)')
    bare = gpu_map(ops, 'six', scans, 1.0, observations=False)
    res = bare.query(pts, poses, sigma=SIGMA, neighbors=7, min_scans=1, max_d2=MAX_D2)
    assert res.scans is None and res.first is None and res.last is None
    want = QR.batch(table, None, clouds, poses, sigma=SIGMA, neighbors=7, min_scans=1, max_d2=MAX_D2)
    for k in ('labels', 'best', 'counts', 'pairs', 'tallies'):
        assert np.array_equal(getattr(res, k).cpu().numpy(), want[k]), k
    for bad in (dict(min_scans=2), dict(outputs=('scans',)), dict(outputs=('labels', 'last'))):
        with pytest.raises(ValueError, match='needs a map created with observations=True'):
            bare.query(pts, poses, **bad)


# ---- the gates, min_points, and the map is only read -------------------------------------------------------------------------------

def test_gated_rows_get_their_labels_and_the_tallies_are_the_maps_skip_counters(ops):
    rows = special_rows()
    far = np.eye(4)
    far[:3, 3] = [0.0, 0.0, 0.3 * 2 ** 20 - 1.0]  # the pose puts a row with z >= 1 beyond the extent
    clouds, poses = [rows, rows[::-1].copy()], np.stack([np.eye(4), far])
    vmap = ops.VoxelMap(0.3, channels=4, capacity=256, moments=True, observations=True).integrate([dev(c) for c in clouds], poses, 5.0, 80.0)
    table, observed = MR.build(clouds, poses, 0.3, 4, 5.0, 80.0), OR.build(clouds, poses, 0.3, 4, 5.0, 80.0)
    ref = QR.batch(table, observed, clouds, poses, sigma=SIGMA, min_range=5.0, max_range=80.0)
    assert {QR.NONFINITE, QR.RANGE, QR.EXTENT, QR.STATIC} <= set(ref['labels'].tolist())
    res = vmap.query([dev(c) for c in clouds], poses, sigma=SIGMA, min_range=5.0, max_range=80.0)
    for k in QR.INTEGERS + ('tallies',):
        assert np.array_equal(getattr(res, k).cpu().numpy(), ref[k]), k
    stats, t = vmap.stats(), res.tallies.sum(0).tolist()
    assert t[:3] == [stats['skipped_nonfinite'], stats['skipped_range'], stats['out_of_extent']] and sum(t[3:7]) == stats['integrated']
    gated = ref['labels'] < QR.UNMAPPED
    assert np.isinf(res.d2.cpu().numpy()[gated]).all() and (res.best.cpu().numpy()[gated] == -1).all()


def test_min_points_boundary_and_nothing_is_written_to_the_map(ops, scans):
    import torch
    cloud = np.float32([[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.5, 0.6, 0.4], [2.5, 0.5, 0.5]])
    vmap = ops.VoxelMap(1.0, channels=3, capacity=64, moments=True, observations=True).integrate([dev(cloud)], np.eye(4)[None])
    q = dev(np.float32([[0.4, 0.4, 0.4], [2.4, 0.5, 0.5]]))
    for min_points, labels in ((3, [QR.STATIC, QR.UNMAPPED]), (4, [QR.UNMAPPED, QR.UNMAPPED]), (1, [QR.STATIC, QR.STATIC])):
        res = vmap.query([q], np.eye(4)[None], sigma=0.5, min_points=min_points)
        assert res.labels.tolist() == labels and res.pairs.tolist() == [int(v == QR.STATIC) for v in labels]
        assert res.counts.tolist() == [3 if labels[0] == QR.STATIC else 0, 1 if labels[1] == QR.STATIC else 0]
    clouds, poses, _ = data('six', scans)
    big = shared_map(ops, 'six', scans, 0.3)
    before = [t.clone() for t in (big._buf, big._mom, big._obs)]
    big.query([dev(c) for c in clouds], poses, sigma=SIGMA, neighbors=7, min_scans=2, max_d2=MAX_D2)
    big.clean([dev(c) for c in clouds], poses, min_scans=2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (big._buf, big._mom, big._obs)))


# ---- clean -------------------------------------------------------------------------------------------------------------------------

def test_clean_returns_the_static_rows_with_all_their_columns(ops, scans, tmp_path):
    import torch
    from rdmnet_amd import trajectory
    clouds, poses, _ = data('six', scans)
    vmap = shared_map(ops, 'six', scans, 0.3)
    wide = [np.concatenate([c, np.arange(len(c) * 2, dtype=np.float32).reshape(-1, 2)], 1) for c in clouds]  # six columns, four channels
    kw = dict(sigma=SIGMA, neighbors=7, min_scans=2, max_d2=MAX_D2)
    ref = reference('six', scans, 0.3, 7)
    kept, tallies = vmap.clean([dev(c) for c in wide], poses, **kw)
    assert np.array_equal(tallies.cpu().numpy(), ref['tallies']) and len(kept) == 6
    off = ref['offsets']
    for k, (got, c) in enumerate(zip(kept, wide)):
        want = c[ref['labels'][off[k]:off[k + 1]] == QR.STATIC]
        assert 0 < len(want) < len(c) and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match='takes no `outputs`'):
        vmap.clean([dev(c) for c in wide], poses, outputs=('labels',))
    # trajectory.clean_scans: the same rows in files of the scans' names and formats, in batches of four
    paths = []
    for k, c in enumerate(clouds):
        paths.append(str(tmp_path / ('%06d' % k + ('.bin' if k % 2 else '.npy'))))
        c.tofile(paths[-1]) if k % 2 else np.save(paths[-1], c)
    got = trajectory.clean_scans(paths, poses, vmap, str(tmp_path / 'clean'), batch=4, **kw)
    assert got.dtype == np.int64 and np.array_equal(got, ref['tallies'])
    for k, c in enumerate(clouds):
        name = tmp_path / 'clean' / os.path.basename(paths[k])
        rows = np.fromfile(name, np.float32).reshape(-1, 4) if k % 2 else np.load(name)
        assert np.array_equal(rows, c[ref['labels'][off[k]:off[k + 1]] == QR.STATIC])


def test_arguments_are_rejected_by_name(ops, scans):
    clouds, poses, _ = data('six', scans)
    vmap = shared_map(ops, 'six', scans, 1.0)
    pts = [dev(clouds[0])]
    for kw, match in ((dict(sigma=0.0), 'sigma must be positive'), (dict(sigma=float('inf')), 'sigma must be positive'),
                      (dict(neighbors=6), 'neighbors must be 1 or 7'), (dict(min_points=0), 'min_points >= 1'),
                      (dict(min_scans=-1), 'min_scans >= 0'), (dict(max_d2=-1.0), 'max_d2 must be >= 0'),
                      (dict(max_d2=float('nan')), 'max_d2 must be >= 0'), (dict(outputs=('labels', 'd3')), "outputs must be among"),
                      (dict(min_range=2.0, max_range=1.0), 'min_range <= max_range')):
        with pytest.raises(ValueError, match=match):
            vmap.query(pts, poses[:1], **kw)
    with pytest.raises(ValueError, match=r'poses must be \[1, 4, 4\]'):
        vmap.query(pts, poses[:2])
    with pytest.raises(ValueError, match='clouds must be a list of tensors'):
        vmap.clean(pts[0], poses[:1])
    empty = vmap.query([], np.zeros((0, 4, 4)))
    assert empty.labels.shape == (0,) and empty.tallies.shape == (0, 8) and empty.scans.shape == (0,)
    none = vmap.query([pts[0][:0]], poses[:1])
    assert none.labels.shape == (0,) and none.tallies.tolist() == [[0] * 8]


# ---- the raw C-ABI ---------------------------------------------------------------------------------------------------------------

def test_raw_abi_argument_errors_and_an_empty_batch(ops, scans):
    import torch
    from rdmnet_amd import _lib
    L = _lib.lib()
    clouds, poses, _ = data('six', scans)
    vmap = shared_map(ops, 'six', scans, 1.0)
    pts = dev(clouds[0])
    n = len(pts)
    off = torch.tensor([0, n], dtype=torch.int64, device='cuda')
    X = torch.from_numpy(poses[:1].copy()).cuda()
    labels = torch.full((n,), 99, dtype=torch.uint8, device='cuda')
    seen = torch.full((n, 3), 99, dtype=torch.int32, device='cuda')
    tallies = torch.full((1, 8), 99, dtype=torch.int64, device='cuda')
    MOM, OBS = (vmap._mom.data_ptr(), vmap._mom.numel()), (vmap._obs.data_ptr(), vmap._obs.numel())

    def call(n_scans=1, total=n, mom=MOM, obs=OBS, sigma=SIGMA, min_points=1, neighbors=1, min_scans=1, max_d2=float('inf'), seen_ptr=0,
             ld=4):
        return L.rdm_voxel_map_query(*vmap._head(), *mom, *obs, vmap.voxel, pts.data_ptr(), ld, total, off.data_ptr(), X.data_ptr(), n_scans,
                                     0.0, float('inf'), sigma, min_points, neighbors, min_scans, max_d2, labels.data_ptr(), 0, 0, seen_ptr,
                                     0, 0, 0, tallies.data_ptr(), _lib.stream_ptr())

    assert call(neighbors=0) == ERR_ARG and call(neighbors=6) == ERR_ARG and b'neighbors must be 1 or 7' in L.rdm_last_error()
    assert call(sigma=0.0) == ERR_ARG and call(sigma=-1.0) == ERR_ARG and b'sigma' in L.rdm_last_error()
    assert call(max_d2=float('nan')) == ERR_ARG and call(max_d2=-1.0) == ERR_ARG and b'max_d2' in L.rdm_last_error()
    assert call(min_points=0) == ERR_ARG and call(min_scans=-1) == ERR_ARG and b'min_points >= 1 and min_scans >= 0' in L.rdm_last_error()
    assert call(n_scans=-1) == ERR_ARG and call(total=-1) == ERR_ARG and call(ld=3) == ERR_ARG and b'bad sizes' in L.rdm_last_error()
    assert call(obs=(0, 0), min_scans=2) == ERR_ARG and b'need an observations block' in L.rdm_last_error()
    assert call(obs=(0, 0), seen_ptr=seen.data_ptr()) == ERR_ARG and b'need an observations block' in L.rdm_last_error()
    assert call(mom=(MOM[0], MOM[1] - 1)) == ERR_ARG and b'moments block is too small' in L.rdm_last_error()
    assert call(obs=(OBS[0], OBS[1] - 1)) == ERR_WORKSPACE and b'observations block is too small' in L.rdm_last_error()
    assert call(n_scans=0) == 0
    torch.cuda.synchronize()
    assert (labels == 99).all() and (seen == 99).all() and (tallies == 99).all()  # nothing ran, n_scans = 0 writes nothing
    assert call(min_scans=2, max_d2=MAX_D2, seen_ptr=seen.data_ptr()) == 0
    want = vmap.query([pts], poses[:1], sigma=SIGMA, min_scans=2, max_d2=MAX_D2)
    assert torch.equal(labels, want.labels) and torch.equal(tallies, want.tallies)
    assert torch.equal(seen, torch.stack([want.scans, want.first, want.last], 1))
    assert call(obs=(0, 0), mom=(0, 0)) == 0  # both blocks are optional
    torch.cuda.synchronize()
    assert torch.equal(labels, vmap.query([pts], poses[:1], sigma=SIGMA).labels)


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_trajectory_map_clean_end_to_end(ops, scans, tmp_path):
    """Four frames of the street with the car under their true poses: --map-clean adds one `clean:` line per variant after the map's
    lines and one directory of cleaned scans, with the restatement's counts and rows; every other line and file is that of a run
    without the flag."""
    from rdmnet_amd import trajectory
    clouds, poses, _ = data('street', scans)
    frames = [0, 3, 6, 9]
    root, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = root / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    for k, f in enumerate(frames):
        np.save(folder / ('%06d.npy' % f), clouds[k])
    for k in range(3):
        T = np.linalg.inv(poses[k + 1]) @ poses[k]
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=T, transform=T, information=np.eye(6))

    def run(name, extra):
        out, lines = tmp_path / name, []
        res = trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(root), '--out', str(out),
                                                                  '--map-min-scans', '2', '--optimize', *extra]), emit=lines.append)
        return lines, out, res

    plain, plain_out, _ = run('plain', [])
    lines, out, res = run('clean', ['--map-clean'])
    assert not any(' clean: ' in s for s in plain) and [s for s in lines if ' clean: ' not in s] == plain
    for name in os.listdir(plain_out):
        assert open(out / name, 'rb').read() == open(plain_out / name, 'rb').read(), name
    assert sorted(set(os.listdir(out)) - set(os.listdir(plain_out))) == ['5_chained_clean', '5_optimized_clean']
    nodes = {'chained': trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0], 'optimized': res.nodes.cpu().numpy()}
    for what, X in nodes.items():
        at = [i for i, s in enumerate(lines) if s.startswith(f'seq 5 {what} ')]
        assert lines[at[-1]].startswith(f'seq 5 {what} clean: ') and f'seq 5 {what} persistent: ' in lines[at[-1] - 1]
        table, observed = MR.build(clouds[:4], X, 0.3, 3), OR.build(clouds[:4], X, 0.3, 3)
        ref = QR.batch(table, observed, clouds[:4], X, sigma=0.02, min_scans=2)
        assert lines[at[-1]] == trajectory.clean_line(5, what, ref['tallies'], 2, np.inf)
        print(lines[at[-1]])
        assert sorted(os.listdir(out / f'5_{what}_clean')) == ['%06d.npy' % f for f in frames]
        for k, f in enumerate(frames):
            keep = ref['labels'][ref['offsets'][k]:ref['offsets'][k + 1]] == QR.STATIC
            assert np.array_equal(np.load(out / f'5_{what}_clean' / ('%06d.npy' % f)), clouds[k][keep])
            assert not keep[-CAR:].any() and keep[:-CAR].any()  # the car is gone, the street is not
    # a finite distance alone is a criterion too, and builds the map with moments
    lines, out, _ = run('d2', ['--map-clean', '--map-clean-max-d2', '25', '--map-clean-neighbors', '7'])
    assert sum('off surface (d2 > 25)' in s for s in lines) == 2
