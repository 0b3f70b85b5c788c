"""GPU: the voxel observations (ops.VoxelMap(observations=True), the raw rdm_voxel_observations_* / rdm_voxel_map_*_observ* /
rdm_voxel_map_prune C-ABI and `python -m rdmnet_amd.trajectory --map-min-scans`) against the NumPy restatement
tests/voxel_observations_restatement.py.  scans, first and last are integers and a pruned map is a subset of the slots of its map, so
everything in this file is compared with np.array_equal or on its bytes: there is no tolerance anywhere."""
import os

import numpy as np
import pytest

import voxel_map_restatement as VM
import voxel_observations_restatement as OR
from test_voxel_map import FACES, random_pose, with_attribute
from test_voxel_map_gpu import RawMap, dev, equal, host, key_of, points_in_cells, special_rows
from test_voxel_moments_gpu import fixture as nearest_300, same_bytes

pytestmark = pytest.mark.gpu

_cache = {}
ERR_ARG, ERR_WORKSPACE = -1, -2  # RDM_ERR_ARG, RDM_ERR_WORKSPACE
EYE = np.eye(4)


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def nudge(rng):
    """A yaw of up to 0.3 rad and a shift of up to 0.4 m (0.04 m in z)."""
    yaw, X = rng.uniform(-0.3, 0.3), np.eye(4)
    X[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    X[:3, 3] = rng.uniform(-0.4, 0.4, 3) * [1.0, 1.0, 0.1]
    return X


def fixture(scans):
    """Six scans -- the 300 points nearest to the sensor of each bundled scan, and every second of them again -- under six poses that
    are a nudge apart, far from the origin and under any rotation, so that voxels are seen in one, two and more scans; and the
    restatement's observations of them at 0.3 m and 1 m: computed once, never changed."""
    if 'clouds' not in _cache:
        rng = np.random.default_rng(31)
        near = nearest_300(scans)[0]
        clouds = list(near) + [c[::2].copy() for c in near]
        base = random_pose(rng)
        poses = np.stack([base @ nudge(rng) for _ in clouds])
        ref = {v: OR.build(clouds, poses, v) for v in (0.3, 1.0)}
        for v in ref:
            assert {1, 2, 3} <= set(ref[v].scans.tolist()), 'the fixture must have voxels seen once and several times'
        _cache['clouds'] = (clouds, poses, ref)
    return _cache['clouds']


def observed_equal(got, want, what=''):
    """(scans, first, last) value for value, dtypes and shapes included."""
    assert len(got) == len(want) == 3
    for g, w, name in zip(got, want, ('scans', 'first', 'last')):
        assert g.dtype == w.dtype == np.int32 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), f'{what} {name}: {int((g != w).sum())} of {g.size} values differ'


def subset(ref, cells):
    """The restatement's (scans, first, last) of the given cells, in the given order."""
    key = np.array([key_of(tuple(int(v) for v in c)) for c in cells], np.uint64)
    pos = np.searchsorted(ref.map.keys, key)
    assert np.array_equal(ref.map.keys[pos], key)
    return tuple(v[pos].astype(np.int32) for v in (ref.scans, ref.first, ref.last))


@pytest.mark.parametrize('voxel', [0.3, 1.0])
def test_scans_under_random_poses(ops, scans, voxel):
    clouds, poses, ref = fixture(scans)
    m = ops.VoxelMap(voxel, capacity=4096, observations=True).integrate([dev(c) for c in clouds], poses)
    got, want = host(m.extract_observations()), ref[voxel].extract()
    observed_equal(got, want)
    equal(host(m.extract()), ref[voxel].map.extract())
    assert m.stats() == ref[voxel].map.stats() and m.capacity == 4096 and m.num_scans == len(clouds) == ref[voxel].num_scans
    print(f'voxel {voxel}: {len(want[0])} voxels, seen in {np.bincount(want[0])[1:].tolist()} voxels by 1, 2, ... scans')
    # min_points selects the matching rows
    counts = ref[voxel].map.counts
    sub, keep = host(m.extract_observations(min_points=4)), counts >= 4
    assert 0 < keep.sum() < len(keep)
    observed_equal(sub, tuple(g[keep] for g in got))
    observed_equal(sub, ref[voxel].extract(4))


def test_one_call_single_scan_calls_and_chunks_are_one_result(ops, scans):
    import torch
    clouds, poses, ref = fixture(scans)
    want, stats = ref[0.3].extract(), ref[0.3].map.stats()
    d = [dev(c) for c in clouds]
    new = lambda **kw: ops.VoxelMap(0.3, capacity=4096, observations=True, **kw)
    forms = {}
    forms['one call, packed'] = new().integrate((torch.cat(d), torch.tensor([0] + [len(c) for c in clouds], dtype=torch.int64).cumsum(0)), poses)
    single = new()
    for c, X in zip(d, poses):
        single.integrate([c], X)
    forms['one scan per call'] = single
    forms['chunks of 2 and 4'] = new().integrate(d[:2], poses[:2]).integrate(d[2:], poses[2:])
    forms['with moments'] = new(moments=True).integrate(d[:5], poses[:5]).integrate(d[5:], poses[5:])
    for name, m in forms.items():
        observed_equal(host(m.extract_observations()), want, name)
        assert m.stats() == stats and m.num_scans == 6, name
    single.reset()
    assert single.num_scans == 0 and len(single) == 0 and all(len(t) == 0 for t in single.extract_observations())
    observed_equal(host(single.integrate(d, poses).extract_observations()), want, 'after reset')  # a reset map is a new map


def test_two_calls_into_the_same_voxels_and_empty_scans(ops, scans):
    """The same scan in two calls: every voxel sees two scans, which it would not if the first call's mask were still set."""
    import torch
    clouds, poses, _ = fixture(scans)
    c, X = dev(clouds[0]), poses[0]
    empty = torch.zeros((0, 4), dtype=torch.float32, device='cuda')
    m = ops.VoxelMap(0.3, capacity=4096, observations=True).integrate([c], X).integrate([c], X)
    scans_, first, last = host(m.extract_observations())
    assert len(scans_) > 100 and (scans_ == 2).all() and (first == 0).all() and (last == 1).all()
    # an empty scan, an empty batch of two and a batch without scans: the ids go on from 2 + 1 + 2 + 0
    m.integrate([empty, c], np.stack([EYE, X])).integrate([empty, empty], [EYE, EYE]).integrate([], np.zeros((0, 4, 4))).integrate([c], X)
    assert m.num_scans == 7
    ref = OR.Observed(0.3).integrate([clouds[0]] * 2, [X] * 2).integrate([clouds[0][:0], clouds[0]], [EYE, X])
    ref.integrate([clouds[0][:0]] * 2, [EYE] * 2).integrate([clouds[0]], [X])
    observed_equal(host(m.extract_observations()), ref.extract())
    assert sorted(set(ref.last.tolist())) == [6] and sorted(set(ref.scans.tolist())) == [4]


def test_64_scans_in_one_call_and_65_through_the_class(ops):
    p, q = np.float32([[0.5, 0.5, 0.5]]), np.float32([[5.5, 0.5, 0.5]])
    for n in (64, 65):
        clouds = [p] + [q] * (n - 2) + [p]
        ref = OR.build(clouds, [EYE] * n, 1.0, channels=3)
        m = ops.VoxelMap(1.0, channels=3, capacity=64, observations=True).integrate([dev(c) for c in clouds], [EYE] * n)
        got = host(m.extract_observations())
        observed_equal(got, ref.extract())
        assert [g.tolist() for g in got] == [[2, n - 2], [0, 1], [n - 1, n - 2]] and m.num_scans == n  # (bit 63; the second call's bit 0)
        equal(host(m.extract()), ref.map.extract())


# ---- the raw C-ABI -------------------------------------------------------------------------------------------------------------

class RawObserved(RawMap):
    """A table that is never grown, with its observations block (and, asked for, a moments block) beside it."""

    def __init__(self, capacity, channels, voxel, moments=False):
        super().__init__(capacity, channels, voxel)
        nbytes = self.L.rdm_voxel_observations_bytes(capacity)
        assert nbytes >= 20 * capacity
        self.obs = self.torch.empty((nbytes,), dtype=self.torch.uint8, device='cuda')
        assert self.L.rdm_voxel_observations_reset(self.obs.data_ptr(), nbytes, capacity, self._lib.stream_ptr()) == 0
        self.mom = None
        if moments:
            self.mom = self.torch.empty((self.L.rdm_voxel_moments_bytes(capacity),), dtype=self.torch.uint8, device='cuda')
            assert self.L.rdm_voxel_moments_reset(self.mom.data_ptr(), self.mom.numel(), capacity, self._lib.stream_ptr()) == 0

    def integrate_observed(self, clouds, poses, first_id=0, short=0):
        pts = dev(np.concatenate(clouds))
        off = dev(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), np.int64)
        X = dev(np.asarray(poses, np.float64).reshape(-1, 16), np.float64)
        mom = (self.mom.data_ptr(), self.mom.numel()) if self.mom is not None else (0, 0)
        return self.L.rdm_voxel_map_integrate_observed(*self.head, self.voxel, pts.data_ptr(), pts.shape[1], pts.shape[0], off.data_ptr(),
                                                       X.data_ptr(), len(clouds), 0.0, float('inf'), *mom, self.obs.data_ptr(),
                                                       self.obs.numel() - short, first_id, self._lib.stream_ptr())

    def extract_observations(self, min_points=1, short=0):
        torch, S = self.torch, self.capacity
        out = [torch.empty((S,), dtype=torch.int32, device='cuda') for _ in range(3)]
        n = torch.zeros((1,), dtype=torch.int64, device='cuda')
        ws = torch.empty((self.L.rdm_voxel_map_extract_workspace_bytes(S),), dtype=torch.uint8, device='cuda')
        rc = self.L.rdm_voxel_map_extract_observations(*self.head, self.obs.data_ptr(), self.obs.numel() - short, self.voxel, min_points,
                                                       *(t.data_ptr() for t in out), S, n.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       self._lib.stream_ptr())
        if rc != 0:
            return rc
        m = int(n.item())
        return host(tuple(t[:m] for t in out))


def test_raw_abi_limits_are_refused_with_the_stated_error():
    rng = np.random.default_rng(3)
    pts = points_in_cells(np.array([[0, 0, 0], [-1, 2, 0]]), 10, 0.5, rng)
    one = [pts[:1]] * 65
    m = RawObserved(64, 4, 0.5)
    assert m.L.rdm_voxel_observations_bytes(63) == 0 and m.L.rdm_voxel_observations_bytes(64) >= 64 * 20
    assert m.integrate_observed(one, [EYE] * 65) == ERR_ARG and b'at most 64 scans' in m.L.rdm_last_error()
    assert m.integrate_observed([pts], [EYE], first_id=-1) == ERR_ARG
    assert m.integrate_observed([pts], [EYE], first_id=OR.MAX_ID) == ERR_ARG
    assert m.integrate_observed(one[:64], [EYE] * 64, first_id=OR.MAX_ID - 63) == ERR_ARG  # the last scan's id would be 2^31 - 1
    assert m.integrate_observed([pts], [EYE], short=1) == ERR_WORKSPACE and b'observations block is too small' in m.L.rdm_last_error()
    assert m.extract_observations(short=8) == ERR_WORKSPACE
    assert m.L.rdm_voxel_observations_reset(m.obs.data_ptr(), m.obs.numel() - 1, 64, m._lib.stream_ptr()) == ERR_WORKSPACE
    big = RawObserved(128, 4, 0.5)
    args = (*m.head[:3], m.obs.data_ptr(), m.obs.numel(), *big.head[:3], big.obs.data_ptr())
    assert m.L.rdm_voxel_observations_rehash(*args, big.obs.numel() - 1, 4, m._lib.stream_ptr()) == ERR_WORKSPACE
    assert m.L.rdm_voxel_map_prune(*m.head[:3], m.obs.data_ptr(), m.obs.numel() - 1, *big.head[:3], 4, 1, 2, m._lib.stream_ptr()) == ERR_WORKSPACE
    assert m.L.rdm_voxel_map_prune(*big.head[:3], big.obs.data_ptr(), big.obs.numel(), *m.head[:3], 4, 1, 2, m._lib.stream_ptr()) == ERR_ARG
    assert m.stats()['integrated'] == 0 and len(m.extract_observations()[0]) == 0  # nothing ran
    # the same calls inside the limits: the largest id, 64 scans, and the rehash into 128 slots
    assert m.integrate_observed(one[:64], [EYE] * 64, first_id=OR.MAX_ID - 64) == 0
    assert m.integrate_observed([pts, pts[:10]], [EYE] * 2, first_id=7) == 0
    ref = OR.Observed(0.5).integrate(one[:64], [EYE] * 64, first_id=OR.MAX_ID - 64).integrate([pts, pts[:10]], [EYE] * 2, first_id=7)
    observed_equal(m.extract_observations(), ref.extract())
    assert ref.last.max() == OR.MAX_ID - 1 and ref.scans.max() >= 65
    assert m.L.rdm_voxel_map_rehash(*m.head[:3], *big.head[:3], 4, m._lib.stream_ptr()) == 0
    assert m.L.rdm_voxel_observations_rehash(*args, big.obs.numel(), 4, m._lib.stream_ptr()) == 0
    observed_equal(big.extract_observations(), ref.extract())
    other = points_in_cells(np.array([[5, 5, 5], [0, 0, 0]]), 7, 0.5, rng)
    assert big.integrate_observed([other], [EYE], first_id=3) == 0  # a slot the rehash did not fill starts from nothing
    observed_equal(big.extract_observations(), ref.integrate([other], [EYE], first_id=3).extract())


def test_raw_abi_table_full_holds_the_restatements_values_for_the_keys_it_kept():
    """200 distinct voxels from two scans into 64 slots, sized as test_voxel_map_gpu's test of the full table: what the table stores
    for a key is the restatement's voxel of that key, and a dropped point observed nothing."""
    rng = np.random.default_rng(6)
    cells = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-2, 3), np.arange(4), indexing='ij'), -1).reshape(-1, 3)
    pts = points_in_cells(cells, 20, 0.3, rng)
    halves = [pts[:150], pts[150:]]  # the first scan reaches about half of the voxels
    ref = OR.build(halves, [EYE] * 2, 0.3)
    assert len(ref.map.keys) == 200 and {1, 2} <= set(ref.scans.tolist())
    m = RawObserved(64, 4, 0.3, moments=True)
    assert m.integrate_observed(halves, [EYE] * 2) == 0
    got, obs, st = m.extract(), m.extract_observations(), m.stats()
    assert st['occupied'] == 64 and len(got[1]) == 64 and st['dropped_full'] > 0
    equal(got, ref.map.subset(got[2]))
    observed_equal(obs, subset(ref, got[2]))
    # prune at two scans into a table of the same size: the kept slots, counted
    keep = obs[0] >= 2
    assert 0 < keep.sum() < 64
    small = RawObserved(64, 4, 0.3)
    assert m.L.rdm_voxel_map_prune(*m.head[:3], m.obs.data_ptr(), m.obs.numel(), *small.head[:3], 4, 1, 2, m._lib.stream_ptr()) == 0
    assert m.L.rdm_voxel_observations_rehash(*m.head[:3], m.obs.data_ptr(), m.obs.numel(), *small.head[:3], small.obs.data_ptr(),
                                             small.obs.numel(), 4, m._lib.stream_ptr()) == 0
    equal(small.extract(), tuple(g[keep] for g in got))
    observed_equal(small.extract_observations(), tuple(g[keep] for g in obs))
    assert small.stats() == dict(st, occupied=int(keep.sum()), integrated=int(got[1][keep].sum()))


@pytest.mark.parametrize('n_scans', [1, 64])
def test_contention_65536_points_in_one_voxel(ops, n_scans):
    rng = np.random.default_rng(n_scans)
    n = 65536
    pts = (rng.uniform(0.0, 0.29, (n, 3)) + [0.3, 0.0, 0.0]).astype(np.float32)
    X = np.eye(4)
    X[:3, 3] = [-299.7, 150.0, 3.0]
    m = ops.VoxelMap(0.3, channels=3, capacity=1 << 17, observations=True)
    m.integrate([dev(c) for c in np.split(pts, n_scans)], [X] * n_scans)
    got = host(m.extract_observations())
    assert [g.tolist() for g in got] == [[n_scans], [0], [n_scans - 1]]
    assert host(m.extract())[1].tolist() == [n] and m.stats()['integrated'] == n and m.capacity == 1 << 17


def test_growth_from_64_slots_in_mid_sequence(ops, scans):
    clouds, poses, ref = fixture(scans)
    small = ops.VoxelMap(0.3, capacity=64, moments=True, observations=True)
    seen = {small.capacity}
    for c, X in zip(clouds, poses):
        small.integrate([dev(c)], [X])  # (a scan comes whole)
        seen.add(small.capacity)
    large = ops.VoxelMap(0.3, capacity=4096, moments=True, observations=True).integrate([dev(c) for c in clouds], poses)
    assert len(seen) >= 3 and large.capacity == 4096, sorted(seen)
    observed_equal(host(small.extract_observations()), ref[0.3].extract())
    observed_equal(host(large.extract_observations()), ref[0.3].extract())
    same_bytes(host(small.extract_moments()), host(large.extract_moments()))
    equal(host(small.extract()), ref[0.3].map.extract())
    assert small.stats() == large.stats() == ref[0.3].map.stats() and small.stats()['dropped_full'] == 0


def test_special_rows_observe_nothing(ops):
    rows = special_rows()
    far = np.eye(4)
    far[0, 3] = 314572.8 - 50.0  # the row at x = 60 leaves the extent under this pose
    origin = np.zeros((1, 4), np.float32)
    faces = []
    for t in FACES:
        X = np.eye(4)
        X[1, 3] = t
        faces.append(X)
    bad = np.float32([[np.nan, 1, 1, 0.5], [1, 1, 1, np.inf], [90, 0, 0, 0.5]])  # a scan whose every row is skipped
    clouds = [rows, rows, bad, rows[::-1].copy()] + [origin] * 4
    poses = np.stack([EYE, far, EYE, EYE] + faces)
    ref = OR.Observed(0.3).integrate(clouds, poses, min_range=0.0, max_range=80.0)
    m = ops.VoxelMap(0.3, capacity=64, observations=True).integrate([dev(c) for c in clouds], poses, max_range=80.0)
    got = host(m.extract_observations())
    observed_equal(got, ref.extract())
    equal(host(m.extract()), ref.map.extract())
    st = m.stats()
    assert st == ref.map.stats() and st['skipped_nonfinite'] == 17 and st['out_of_extent'] >= 3 and st['skipped_range'] == 4
    assert 2 not in set(got[1].tolist()) | set(got[2].tolist()) and m.num_scans == 8  # nothing saw scan 2, which still has its id
    assert got[0].max() >= 2  # the rows of scans 0 and 3 share their voxels


def test_the_base_map_and_the_moments_are_unchanged_by_the_observations(ops, scans):
    clouds, poses, _ = fixture(scans)
    d = [dev(c) for c in clouds]
    plain = ops.VoxelMap(0.3, capacity=4096, moments=True).integrate(d, poses)
    observed = ops.VoxelMap(0.3, capacity=4096, moments=True, observations=True).integrate(d, poses)
    assert plain._obs is None and observed._obs is not None and plain.num_scans == 0
    for min_points in (1, 3):
        equal(host(observed.extract(min_points)), host(plain.extract(min_points)))
        same_bytes(host(observed.extract_moments(min_points)), host(plain.extract_moments(min_points)))
    assert observed.stats() == plain.stats() and observed._buf.numel() == plain._buf.numel() and observed._mom.numel() == plain._mom.numel()
    equal(host(ops.VoxelMap(0.3, capacity=4096, observations=True).integrate(d, poses).extract()), host(plain.extract()))
    for bad in (plain.extract_observations, lambda: plain.pruned(2)):
        with pytest.raises(ValueError, match='observations=True'):
            bad()
    with pytest.raises(ValueError, match='min_scans'):
        observed.pruned(-1)


# ---- the pruned map --------------------------------------------------------------------------------------------------------------

def all_of(m, min_points=1):
    return host(m.extract(min_points)), host(m.extract_moments(min_points)), host(m.extract_observations(min_points))


@pytest.mark.parametrize('voxel', [0.3, 1.0])
def test_pruned_is_the_masked_rows_of_its_map_and_a_map_of_the_persistent_points(ops, scans, voxel):
    clouds, poses, ref = fixture(scans)
    d = [dev(c) for c in clouds]
    new = lambda: ops.VoxelMap(voxel, capacity=4096, moments=True, observations=True)
    full = new().integrate(d, poses)
    before = all_of(full), full.stats()
    pruned = full.pruned(2)
    keep = ref[voxel].keep(2)
    assert 0 < keep.sum() < len(keep)
    (pts, mom, obs), st = before
    got = all_of(pruned)
    equal(got[0], tuple(g[keep] for g in pts))
    same_bytes(got[1], tuple(g[keep] for g in mom))
    observed_equal(got[2], tuple(g[keep] for g in obs))
    assert pruned.stats() == dict(st, occupied=int(keep.sum()), integrated=int(pts[1][keep].sum())) == ref[voxel].pruned(2).map.stats()
    assert (pruned.capacity, pruned.moments, pruned.observations, pruned.num_scans) == (4096, True, True, 6)
    # the map itself is only read
    after = all_of(full), full.stats()
    assert after[1] == st and all(a.tobytes() == b.tobytes() for x, y in zip(after[0], before[0]) for a, b in zip(x, y))
    # min_points takes part, and extract's own min_points selects among what was kept
    keep3 = ref[voxel].keep(2, min_points=3)
    assert 0 < keep3.sum() < keep.sum()
    equal(host(full.pruned(2, min_points=3).extract()), tuple(g[keep3] for g in pts))
    equal(host(pruned.extract(3)), tuple(g[keep3] for g in pts))
    assert len(full.pruned(7)) == 0 and len(full.pruned(1)) == len(keep) == len(full.pruned(0, 0))
    # a map without moments
    bare = ops.VoxelMap(voxel, capacity=4096, observations=True).integrate(d, poses).pruned(2)
    assert bare._mom is None
    equal(host(bare.extract()), got[0])
    # ... and equal to a fresh map integrated from only the points that lie in persistent voxels (a scan left empty keeps its id)
    persistent = ref[voxel].map.keys[keep]
    parts = []
    for c, X in zip(clouds, poses):
        key = VM.quantise(c, X, voxel, 4)[0]
        assert len(key) == len(c)  # (no row of the fixture is skipped)
        parts.append(c[np.isin(key, persistent)])
    fresh = new().integrate([dev(c) for c in parts], poses)
    want = all_of(fresh)
    equal(got[0], want[0])
    same_bytes(got[1], want[1])
    observed_equal(got[2], want[2])
    assert pruned.stats() == fresh.stats()
    # ... so that a registration against either is the same registration, bit for bit
    moved = poses[1] @ np.array([[np.cos(0.01), -np.sin(0.01), 0.0, 0.03], [np.sin(0.01), np.cos(0.01), 0.0, -0.02], [0.0, 0.0, 1.0, 0.01],
                                 [0.0, 0.0, 0.0, 1.0]])
    a, b = (m.register([d[1]], moved[None], sigma=0.05, min_points=3, neighbors=7, max_iteration=5) for m in (pruned, fresh))
    for name in ('transformations', 'information', 'gradient', 'cost', 'iterations', 'num_correspondences', 'num_points', 'status'):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.tobytes() == y.tobytes(), name
    assert int(a.num_correspondences[0]) > 0
    c = full.register([d[1]], moved[None], sigma=0.05, min_points=3, neighbors=7, max_iteration=5)
    assert int(c.num_correspondences[0]) >= int(a.num_correspondences[0])  # (the full map has no less to match against)
    # a pruned map goes on as any map: it is integrated into, grows and is pruned again
    more = pruned.integrate([d[0]], poses[:1])
    assert more.num_scans == 7 and int(host(more.extract_observations())[2].max()) == 6


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_trajectory_map_min_scans_end_to_end(ops, scans, tmp_path):
    """Three frames of one tiny scan seen from known poses, each with a box of its own somewhere else above the scene: without the new
    flags the lines and the files are those of a run that names the defaults; with --map-min-scans 2 the boxes are gone from the written
    map, the `map:` and `sharpness:` lines describe the pruned map and a `persistent:` line follows the `map:` line."""
    from rdmnet_amd import trajectory
    rng = np.random.default_rng(9)
    world = with_attribute(scans['s000000'][:3000], 3)
    X = [np.eye(4), random_pose(rng, 3.0), random_pose(rng, 6.0)]
    data, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    frames = [0, 4, 9]
    boxes = []
    for k, (f, Xk) in enumerate(zip(frames, X)):
        box = np.concatenate([rng.integers(0, 2, (200, 3)) + rng.uniform(0.1, 0.9, (200, 3)) + [10.0 * k - 10.0, 3.0, 40.0],
                              rng.uniform(0.0, 1.0, (200, 1))], 1).astype(np.float32)  # eight voxels, no point near a face
        boxes.append(box)
        both = np.concatenate([world, box])
        inv = np.linalg.inv(Xk)
        local = both.copy()
        local[:, :3] = (both[:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        np.save(folder / ('%06d.npy' % f), local)
    for k in range(2):
        T = np.linalg.inv(X[k + 1]) @ X[k]
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=T, transform=T, information=np.eye(6))

    def run(name, extra):
        out, lines = tmp_path / name, []
        trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                            '--map-voxel', '1.0', '--map-sharpness', *extra]), emit=lines.append)
        return lines, {n: open(out / n, 'rb').read() for n in sorted(os.listdir(out))}

    plain, plain_files = run('plain', [])
    named, named_files = run('named', ['--map-min-scans', '1'])
    assert named == plain and named_files == plain_files and not any(' persistent: ' in s for s in plain)
    nodes = trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0]
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    vmap = trajectory.build_map(paths, nodes, voxel=1.0, moments=True)
    assert vmap.observations is False
    pts, counts, _ = host(vmap.extract())
    assert plain_files['5_chained_map.npy'] == open_bytes(tmp_path, np.concatenate([pts, counts[:, None].astype(np.float32)], 1))

    lines, files = run('two', ['--map-min-scans', '2'])
    full = trajectory.build_map(paths, nodes, voxel=1.0, moments=True, observations=True)
    pruned = full.pruned(2)
    pts, counts, cells = host(pruned.extract())
    assert files['5_chained_map.npy'] == open_bytes(tmp_path, np.concatenate([pts, counts[:, None].astype(np.float32)], 1))
    assert sorted(files) == sorted(plain_files) and files['5_chained.txt'] == plain_files['5_chained.txt']
    at = [i for i, s in enumerate(lines) if ' map: ' in s]
    assert len(at) == 1 and lines[:at[0]] == plain[:at[0]]
    assert lines[at[0]] == trajectory.map_line(5, 'chained', 1.0, len(counts), int(counts.sum()), pruned.stats())
    assert lines[at[0] + 1] == trajectory.persistent_line(5, 'chained', 2, pruned.stats(), full.stats(), 3)
    assert lines[at[0] + 2] == trajectory.sharpness_line(5, 'chained', 4, pruned.sharpness(4)) and len(lines) == len(plain) + 1
    # what was removed: every voxel of the boxes; what was kept: seen in two scans at least, as the restatement has it
    ref = OR.build([np.load(p) for p in paths], nodes, 1.0)
    assert np.array_equal(cells, ref.map.extract()[2][ref.keep(2)]) and len(counts) < len(ref.map.keys)
    box_keys = np.unique(np.concatenate([VM.quantise(b, EYE, 1.0, 4)[0] for b in boxes]))
    kept_keys = np.array([key_of(tuple(int(v) for v in c)) for c in cells], np.uint64)
    assert len(box_keys) == 3 * 8 and not np.isin(box_keys, kept_keys).any() and np.isin(box_keys, ref.map.keys).all()
    print(lines[at[0] + 1])
    # the refinement against the persistent voxels, with every variant's map pruned
    refined, _ = run('refine', ['--map-min-scans', '2', '--map-refine', '--map-refine-min-scans', '2'])
    assert sum(' persistent: ' in s for s in refined) == 2 and any(s.startswith('seq 5 refined persistent: ') for s in refined)
    assert any(s.startswith('seq 5 refined against the map: 3 frames, ') for s in refined)


def open_bytes(tmp_path, array):
    """The bytes of np.save(array)."""
    path = tmp_path / 'expected.npy'
    np.save(path, array)
    return open(path, 'rb').read()
