"""GPU: the voxel map state (ops.VoxelMap.state / from_state / save / load / merge, the raw rdm_voxel_map_export / rdm_voxel_map_import
C-ABI and `python -m rdmnet_amd.trajectory --map-save / --map-prior / --map-localize`) against the NumPy restatement
tests/voxel_state_restatement.py.  The state is integers and a reloaded or merged map is the same integers in other slots, so everything
in this file is compared with np.array_equal, torch.equal or on its bytes; the two tolerances of the localisation test are the nine
decimals of a pose file and tests/test_voxel_register_gpu.py's POSE_BOUND against the restatement's differently ordered sums."""
import ctypes
import os

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_query_restatement as QR
import voxel_register_restatement as RR
import voxel_state_restatement as SR
from test_voxel_map_gpu import RawMap, dev, fmix64, host, special_rows
from test_voxel_observations_gpu import fixture as six_scans
from test_voxel_query import CAR, scene
from test_voxel_register import perturb, pose_error
from test_voxel_register_gpu import POSE_BOUND, outputs

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -1, -2  # RDM_ERR_ARG, RDM_ERR_WORKSPACE
KINDS = (dict(moments=False, observations=False), dict(moments=True, observations=False), dict(moments=False, observations=True),
         dict(moments=True, observations=True))
NAMES = ('keys', 'counts', 'sums', 'moments', 'observations')


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def arrays(state):
    """The arrays of a state (ops.VoxelMap.state's dict, or the restatement's export) as numpy, None where it has none."""
    return {k: None if state.get(k) is None else (state[k] if isinstance(state[k], np.ndarray) else state[k].cpu().numpy()) for k in NAMES}


def same_arrays(got, want, what=''):
    got, want = arrays(got), arrays(want)
    for k in NAMES:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
            assert np.array_equal(got[k], want[k]), f'{what} {k}: {int((got[k] != want[k]).sum())} of {want[k].size} values differ'


def same_map(got, want, what=''):
    """Two ops.VoxelMap hold the same map: every export, the six counters, num_scans."""
    assert (got.moments, got.observations) == (want.moments, want.observations), what
    same_arrays(got.state(), want.state(), what)
    assert got.stats() == want.stats() and got.num_scans == want.num_scans, (what, got.stats(), want.stats(), got.num_scans, want.num_scans)


def gpu_map(ops, clouds, poses, voxel, channels=4, capacity=1 << 12, **kw):
    kind = {k: kw.pop(k) for k in ('moments', 'observations') if k in kw}
    return ops.VoxelMap(voxel, channels=channels, capacity=capacity, **kind).integrate([dev(c) for c in clouds], poses, **kw)


# ---- export ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('voxel', [0.3, 1.0])
@pytest.mark.parametrize('channels', [3, 4])
def test_export_against_the_restatement(ops, scans, channels, voxel):
    import torch
    clouds, poses, _ = six_scans(scans)
    for kind in KINDS:
        ref = SR.build(clouds, poses, voxel, channels, **kind)
        m = gpu_map(ops, clouds, poses, voxel, channels, **kind)
        for min_points in (1, 3):
            st, want = m.state(min_points), SR.export(ref, min_points)
            same_arrays(st, want, f'{kind} min_points {min_points}')
            assert 0 < len(want['keys']) and (min_points == 1 or len(want['keys']) < len(ref.keys))
            # its rows are the rows of extract
            _, counts, cells = m.extract(min_points)
            keys = ((cells[:, 0].long() + SR.VM.HALF) << 42) | ((cells[:, 1].long() + SR.VM.HALF) << 21) | (cells[:, 2].long() + SR.VM.HALF)
            assert torch.equal(st['keys'].view(torch.int64), keys) and torch.equal(st['counts'].view(torch.int32), counts)
            if kind['moments']:
                assert torch.equal(st['moments'], m.extract_moments(min_points)[0])
            if kind['observations']:
                assert torch.equal(st['observations'], torch.stack(m.extract_observations(min_points), 1))
        st = m.state()
        assert (st['voxel'], st['channels'], st['num_scans']) == (voxel, channels, 6 if kind['observations'] else 0)
        assert st['counters'] == m.stats() == ref.stats()


# ---- save and load ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['capacity 64', 'capacity 4096', 'without moments'])
def test_save_and_load_give_the_map_back_bit_for_bit(ops, scans, tmp_path, case):
    import torch
    clouds, poses, _ = six_scans(scans)
    keep = case != 'without moments'
    first = gpu_map(ops, clouds, poses, 0.3, moments=True, observations=True)
    path = first.save(str(tmp_path / 'map_state.npz'))
    assert os.listdir(tmp_path) == ['map_state.npz']
    original = first if keep else gpu_map(ops, clouds, poses, 0.3, moments=False, observations=True)
    options = {'capacity 64': dict(capacity=64), 'capacity 4096': dict(capacity=1 << 12), 'without moments': dict(moments=False)}[case]
    loaded = ops.VoxelMap.load(path, **options)
    rows = len(first)
    assert rows > 100 and loaded.capacity >= 2 * rows  # (64 slots grow)
    assert loaded.capacity == (4096 if case == 'capacity 4096' else min(c for c in (1 << k for k in range(6, 31)) if c >= 2 * rows))
    assert loaded.moments is keep and loaded.observations is True
    same_map(loaded, original, case)
    for a, b in zip(loaded.extract() + loaded.extract_observations(), original.extract() + original.extract_observations()):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
    batch = [dev(clouds[0]), dev(clouds[4])]
    X = np.stack([perturb(poses[0], np.random.default_rng(1), 0.05, 0.005), poses[4]])
    if keep:
        for a, b in zip(loaded.extract_moments(), original.extract_moments()):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        res = [m.register(batch, X, min_points=2) for m in (loaded, original)]
        assert int(res[1].num_correspondences.min()) > 0
        for a, b in zip(outputs(res[0]), outputs(res[1])):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    q = [m.query(batch, X, neighbors=7, min_scans=2, max_d2=25.0) for m in (loaded, original)]
    for name in ops.MapQueryResult.FIELDS:
        a, b = getattr(q[0], name), getattr(q[1], name)
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), name
    assert len(set(q[1].labels.tolist())) >= 2
    # a loaded map is a map: it takes further scans like the original
    more, X = [dev(clouds[1][:100] + np.float32(0.05))], poses[1:2]
    same_map(loaded.integrate(more, X), original.integrate(more, X), case + ', one scan more')
    assert loaded.num_scans == 7
    bare = gpu_map(ops, clouds[:1], poses[:1], 1.0).state()
    with pytest.raises(ValueError, match='moments=True, but the state holds no moments'):
        ops.VoxelMap.from_state(bare, moments=True)
    with pytest.raises(ValueError, match='observations=True, but the state holds no observations'):
        ops.VoxelMap.from_state(bare, observations=True)


def test_a_pruned_map_saves_and_loads_like_any_other(ops, scans, tmp_path):
    clouds, poses, _ = six_scans(scans)
    pruned = gpu_map(ops, clouds, poses, 0.3, moments=True, observations=True).pruned(2)
    loaded = ops.VoxelMap.load(pruned.save(str(tmp_path / 'pruned.npz')))
    same_map(loaded, pruned)
    st = loaded.state()
    assert 0 < len(st['keys']) < len(SR.build(clouds, poses, 0.3, 4).keys) and int(st['observations'][:, 0].min()) == 2
    # a state with a record that no map holds is refused when it is imported
    bad = {k: (v.cpu().numpy().copy() if hasattr(v, 'cpu') else v) for k, v in st.items()}
    bad['counts'][3] = 0
    with pytest.raises(ValueError, match='1 of %d records are not records of a voxel map' % len(st['keys'])):
        ops.VoxelMap.from_state(bad)


# ---- merge -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', KINDS, ids=['plain', 'moments', 'observations', 'both'])
def test_the_merge_law(ops, scans, kind):
    clouds, poses, _ = six_scans(scans)
    part = lambda lo, hi, **kw: gpu_map(ops, clouds[lo:hi], poses[lo:hi], 0.3, **kind, **kw)
    one = part(0, 6)
    ref = SR.build(clouds, poses, 0.3, 4, **kind)
    same_arrays(one.state(), SR.export(ref), 'the one-pass map')
    for k in (1, 3, 5):
        a, b = part(0, k), part(k, 6)
        before = b.state()
        assert a.merge(b) is a
        same_map(a, one, f'split at {k}')
        same_arrays(b.state(), before, 'the merged map is only read')
    same_map(part(0, 2).merge(part(2, 3)).merge(part(3, 6)), one, '(a + b) + c')
    same_map(part(0, 2).merge(part(2, 3).merge(part(3, 6))), one, 'a + (b + c)')
    small = part(0, 1, capacity=64)
    same_map(small.merge(part(1, 6)), one, 'into a map of 64 slots')
    assert small.capacity >= 2 * len(ref.keys) > 128
    if kind['observations']:  # the other order, with the ids said
        empty = ops.VoxelMap(0.3, capacity=64, **kind)
        same_map(empty.merge(part(3, 6), id_offset=3).merge(part(0, 3), id_offset=0), one, 'late scans first')
    # a block that only the other map has is left out
    if kind['moments'] or kind['observations']:
        bare = gpu_map(ops, clouds[:2], poses[:2], 0.3).merge(part(2, 6))
        same_arrays(bare.state(), SR.export(SR.build(clouds, poses, 0.3, 4)), 'into a map without the blocks')


def test_merge_adds_the_skip_counters_of_both_halves(ops):
    rows = special_rows()
    far = np.eye(4)
    far[0, 3] = 314572.8 - 50.0
    clouds, poses = [rows, rows, rows[::-1].copy(), rows[5:]], np.stack([np.eye(4), far, np.eye(4), far])
    kind = dict(moments=True, observations=True)
    one = gpu_map(ops, clouds, poses, 0.3, capacity=64, max_range=80.0, **kind)
    st = one.stats()
    assert st['skipped_nonfinite'] >= 10 and st['skipped_range'] >= 2 and st['out_of_extent'] >= 3 and st['dropped_full'] == 0
    ref = SR.build(clouds, poses, 0.3, 4, max_range=80.0, **kind)
    assert st == ref.stats()
    a = gpu_map(ops, clouds[:2], poses[:2], 0.3, capacity=64, max_range=80.0, **kind)
    b = gpu_map(ops, clouds[2:], poses[2:], 0.3, capacity=64, max_range=80.0, **kind)
    same_map(a.merge(b), one)


def test_merge_refuses_by_name(ops, scans):
    clouds, poses, _ = six_scans(scans)
    a = gpu_map(ops, clouds[:1], poses[:1], 0.3, moments=True, observations=True)
    before = a.state()
    for other, message in ((gpu_map(ops, clouds[:1], poses[:1], 0.3 + 1e-12, moments=True, observations=True), 'voxel differs'),
                           (gpu_map(ops, clouds[:1], poses[:1], 0.3, 3, moments=True, observations=True), 'channels differ'),
                           (gpu_map(ops, clouds[:1], poses[:1], 0.3, observations=True), 'other has no moments'),
                           (gpu_map(ops, clouds[:1], poses[:1], 0.3, moments=True), 'other has no observations'), ('a map', 'must be a VoxelMap')):
        with pytest.raises(ValueError, match='VoxelMap.merge: .*' + message):
            a.merge(other)
    b = gpu_map(ops, clouds[1:2], poses[1:2], 0.3, moments=True, observations=True)
    with pytest.raises(ValueError, match='id_offset must be >= 0'):
        a.merge(b, id_offset=-1)
    with pytest.raises(ValueError, match='ids overflow'):
        a.merge(b, id_offset=2 ** 31 - 1)
    same_arrays(a.state(), before)
    assert a.num_scans == 1 and a.merge(b, id_offset=2 ** 31 - 2).num_scans == 2 ** 31 - 1  # the last id there is


# ---- the raw C-ABI ---------------------------------------------------------------------------------------------------------------

class RawState(RawMap):
    """test_voxel_map_gpu.RawMap with the two optional blocks and the two state calls."""

    def __init__(self, capacity, channels=3, moments=True, observations=True):
        super().__init__(capacity, channels, 1.0)
        torch, L, lib = self.torch, self.L, self._lib
        self.mom = torch.empty((L.rdm_voxel_moments_bytes(capacity),), dtype=torch.uint8, device='cuda') if moments else None
        self.obs = torch.empty((L.rdm_voxel_observations_bytes(capacity),), dtype=torch.uint8, device='cuda') if observations else None
        if moments:
            assert L.rdm_voxel_moments_reset(self.mom.data_ptr(), self.mom.numel(), capacity, lib.stream_ptr()) == 0
        if observations:
            assert L.rdm_voxel_observations_reset(self.obs.data_ptr(), self.obs.numel(), capacity, lib.stream_ptr()) == 0
        self.ws = torch.empty((L.rdm_voxel_map_extract_workspace_bytes(capacity),), dtype=torch.uint8, device='cuda')
        self.rejected = torch.full((1,), -7, dtype=torch.int64, device='cuda')

    def blocks(self, mom=True, obs=True):
        return ((self.mom.data_ptr(), self.mom.numel()) if mom and self.mom is not None else (0, 0)) + \
               ((self.obs.data_ptr(), self.obs.numel()) if obs and self.obs is not None else (0, 0))

    def add(self, keys, counts, sums, moms=None, seen=None, id_offset=0, skipped=None, n=None, head=None, blocks=None, rejected=True):
        """rdm_voxel_map_import of numpy records -> (the return code, *n_rejected)."""
        self.held = [None if a is None else dev(a, dtype)
                     for a, dtype in ((keys, np.uint64), (counts, np.uint32), (sums, np.int64), (moms, np.int64), (seen, np.int32))]
        host_skipped = None if skipped is None else (ctypes.c_uint64 * 4)(*skipped)
        rc = self.L.rdm_voxel_map_import(*(head or self.head), *(self.blocks() if blocks is None else blocks),
                                         *(self._lib.ptr(t) for t in self.held), len(keys) if n is None else n, id_offset,
                                         0 if skipped is None else ctypes.addressof(host_skipped),
                                         self.rejected.data_ptr() if rejected else 0, self._lib.stream_ptr())
        return rc, int(self.rejected.item())

    def export(self, min_points=1, max_rows=None, mom=True, obs=True, outputs=NAMES, ws_bytes=None, blocks=None):
        """rdm_voxel_map_export -> (the return code, dict of numpy arrays cut to min(*n_rows, max_rows), *n_rows)."""
        torch, S, C = self.torch, self.capacity if max_rows is None else max_rows, self.channels
        R = max(S, 1)
        out = dict(keys=torch.zeros((R,), dtype=torch.int64, device='cuda').view(torch.uint64),
                   counts=torch.zeros((R,), dtype=torch.int32, device='cuda').view(torch.uint32),
                   sums=torch.zeros((R, C), dtype=torch.int64, device='cuda'), moments=torch.zeros((R, 9), dtype=torch.int64, device='cuda'),
                   observations=torch.zeros((R, 3), dtype=torch.int32, device='cuda'))
        n = torch.full((1,), -1, dtype=torch.int64, device='cuda')
        rc = self.L.rdm_voxel_map_export(*self.head, *(self.blocks(mom, obs) if blocks is None else blocks), min_points,
                                         *(out[k].data_ptr() if k in outputs else 0 for k in NAMES), S, n.data_ptr(), self.ws.data_ptr(),
                                         self.ws.numel() if ws_bytes is None else ws_bytes, self._lib.stream_ptr())
        m = int(n.item())
        return rc, {k: out[k][:max(min(m, S), 0)].cpu().numpy() if k in outputs else None for k in NAMES}, m


def restated(state):
    return dict(SR.export(state))


def test_raw_abi_65536_records_of_one_key(ops):
    rng = np.random.default_rng(3)
    n = 65536
    keys = np.full(n, (5 << 42) | (1 << 21) | 9, np.uint64)
    counts = rng.integers(1, 1 << 16, n).astype(np.uint32)
    counts[:3] = 0xffffffff  # the count wraps, `integrated` does not
    sums = rng.integers(-2 ** 40, 2 ** 40, (n, 3))
    moms = rng.integers(0, 2 ** 36, (n, 9))
    first = rng.integers(0, 1000, n)
    seen = np.stack([np.ones(n, np.int64), first, first + rng.integers(0, 1000, n)], 1).astype(np.int32)
    ref = SR.State(1.0, 3, True, True)
    assert SR.add_records(ref, keys, counts, sums, moms, seen, id_offset=17) == 0
    m = RawState(64)
    assert m.add(keys, counts, sums, moms, seen, id_offset=17, skipped=(1, 2, 3, 4)) == (0, 0)
    rc, got, rows = m.export()
    assert rc == 0 and rows == 1
    same_arrays(got, restated(ref))
    assert got['observations'].tolist() == [[n, int(first.min()) + 17, int(seen[:, 2].max()) + 17]]
    assert m.stats() == dict(occupied=1, integrated=int(counts.astype(np.int64).sum()), skipped_nonfinite=1, skipped_range=2, out_of_extent=3,
                             dropped_full=4)
    assert int(got['counts'][0]) == m.stats()['integrated'] % 2 ** 32 != m.stats()['integrated']


def test_raw_abi_100_keys_into_64_slots(ops):
    """Two records of each of 100 keys, shuffled: the table stores 64 keys with both of their records and drops the others whole."""
    rng = np.random.default_rng(4)
    keys = np.repeat((rng.permutation(1 << 20)[:100].astype(np.uint64) << np.uint64(21)) | np.uint64(77), 2)
    order = rng.permutation(200)
    keys = keys[order]
    counts = rng.integers(1, 100, 200).astype(np.uint32)
    sums, moms = rng.integers(-2 ** 40, 2 ** 40, (200, 3)), rng.integers(0, 2 ** 36, (200, 9))
    seen = np.stack([np.ones(200, np.int64), order, order], 1).astype(np.int32)
    ref = SR.State(1.0, 3, True, True)
    SR.add_records(ref, keys, counts, sums, moms, seen)
    assert len(ref.keys) == 100
    m = RawState(64)
    assert m.add(keys, counts, sums, moms, seen) == (0, 0)
    rc, got, rows = m.export()
    st = m.stats()
    assert rc == 0 and rows == 64 and st['occupied'] == 64
    at = np.searchsorted(ref.keys, got['keys'])
    assert np.array_equal(ref.keys[at], got['keys'])
    want = restated(ref)
    same_arrays(got, {k: want[k][at] for k in NAMES}, 'the kept keys hold all of their records')
    kept = np.isin(keys, got['keys'])
    assert st['integrated'] == int(counts[kept].sum()) and st['dropped_full'] == int(counts[~kept].sum()) > 0
    assert (got['observations'][:, 0] == 2).all()
    # max_rows below the number of rows: the first rows, and *n_rows still the number there are
    rc, part, rows = m.export(max_rows=10)
    assert rc == 0 and rows == 64
    same_arrays(part, {k: want[k][at][:10] for k in NAMES})
    rc, none, rows = m.export(outputs=())  # every output may be null
    assert rc == 0 and rows == 64


def test_raw_abi_invalid_records_are_counted_and_change_nothing(ops):
    top = 2 ** 31 - 2
    good_key = np.uint64((3 << 42) | (3 << 21) | 3)
    m = RawState(64)
    ok = dict(keys=np.array([good_key, good_key + np.uint64(1)]), counts=np.array([4, 1], np.uint32), sums=np.arange(6).reshape(2, 3) - 2,
              moms=np.arange(18).reshape(2, 9), seen=np.array([[2, 1, 5], [1, top - 5, top - 5]], np.int32))
    assert m.add(**ok, id_offset=5) == (0, 0)
    rc, before, rows = m.export()
    assert rows == 2 and before['observations'].tolist() == [[2, 6, 10], [1, top, top]]
    stats = m.stats()
    bad_keys = np.array([1 << 63, (1 << 64) - 1, good_key, good_key, good_key, good_key, good_key, good_key, good_key], np.uint64)
    bad_counts = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint32)
    bad_seen = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [3, 4, 5], [1, -1, 0], [1, 3, 2], [1, top - 4, top - 4], [-1, 0, 0]], np.int32)
    assert SR.valid(bad_keys, bad_counts, bad_seen, id_offset=5).sum() == 0
    assert m.add(bad_keys, bad_counts, np.ones((9, 3), np.int64), np.ones((9, 9), np.int64), bad_seen, id_offset=5) == (0, 9)
    rc, after, rows = m.export()
    same_arrays(after, before)
    assert m.stats() == stats
    # the same batch among valid records: those are added, *n_rejected is zeroed by every call
    keys, counts = np.concatenate([bad_keys, ok['keys']]), np.concatenate([bad_counts, ok['counts']])
    assert m.add(keys, counts, np.concatenate([np.ones((9, 3), np.int64), ok['sums']]), np.concatenate([np.ones((9, 9), np.int64), ok['moms']]),
                 np.concatenate([bad_seen, ok['seen']]), id_offset=5) == (0, 9)
    rc, twice, rows = m.export()
    assert np.array_equal(twice['counts'], 2 * before['counts']) and np.array_equal(twice['sums'], 2 * before['sums'])
    assert twice['observations'].tolist() == [[4, 6, 10], [2, top, top]]
    assert m.add(**ok, id_offset=5) == (0, 0)


def test_raw_abi_argument_errors_and_an_empty_batch(ops):
    m = RawState(64)
    L = m.L
    ok = dict(keys=np.array([5], np.uint64), counts=np.array([1], np.uint32), sums=np.zeros((1, 3), np.int64), moms=np.zeros((1, 9), np.int64),
              seen=np.array([[1, 0, 0]], np.int32))
    MOM, OBS = m.blocks()[:2], m.blocks()[2:]
    assert m.add(**ok, id_offset=-1)[0] == ERR_ARG and b'id_offset' in L.rdm_last_error()
    assert m.add(**ok, n=-1)[0] == ERR_ARG and m.add(**ok, rejected=False)[0] == ERR_ARG and b'n_rejected' in L.rdm_last_error()
    assert m.add(**dict(ok, moms=None))[0] == ERR_ARG and b'moment_sums is required if and only if' in L.rdm_last_error()
    assert m.add(**ok, blocks=(0, 0) + OBS)[0] == ERR_ARG and b'moment_sums is required if and only if' in L.rdm_last_error()
    assert m.add(**dict(ok, seen=None))[0] == ERR_ARG and b'seen is required if and only if' in L.rdm_last_error()
    assert m.add(**ok, blocks=MOM + (0, 0))[0] == ERR_ARG and b'seen is required if and only if' in L.rdm_last_error()
    assert m.add(ok['keys'], ok['counts'], None, ok['moms'], ok['seen'])[0] == ERR_ARG and b'null keys, counts or sums' in L.rdm_last_error()
    assert m.add(**ok, head=(m.head[0], m.head[1], 100, 3))[0] == ERR_ARG and b'power of two' in L.rdm_last_error()
    assert m.add(**ok, head=(m.head[0], m.head[1] - 1, 64, 3))[0] == ERR_WORKSPACE and b'map block is too small' in L.rdm_last_error()
    assert m.add(**ok, blocks=(MOM[0], MOM[1] - 1) + OBS)[0] == ERR_WORKSPACE and b'moments block is too small' in L.rdm_last_error()
    assert m.add(**ok, blocks=MOM + (OBS[0], OBS[1] - 1))[0] == ERR_WORKSPACE and b'observations block is too small' in L.rdm_last_error()
    assert m.stats() == dict.fromkeys(SR.VM.STATS, 0) and m.export()[2] == 0  # nothing ran
    # n_records = 0 is valid: *n_rejected is zeroed and the skip counters are added
    assert m.add(np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 3), np.int64), None, None, skipped=(1, 0, 2, 0)) == (0, 0)
    assert m.stats() == dict(occupied=0, integrated=0, skipped_nonfinite=1, skipped_range=0, out_of_extent=2, dropped_full=0)
    assert m.add(**ok) == (0, 0) and m.export()[2] == 1
    assert m.export(min_points=-1)[0] == ERR_ARG and m.export(max_rows=-1)[0] == ERR_ARG and b'bad min_points, max_rows' in L.rdm_last_error()
    assert m.export(mom=False)[0] == ERR_ARG and b'moment_sums needs a moments block and seen an observations block' in L.rdm_last_error()
    assert m.export(obs=False)[0] == ERR_ARG and b'moment_sums needs a moments block and seen an observations block' in L.rdm_last_error()
    assert m.export(ws_bytes=m.ws.numel() - 1)[0] == ERR_WORKSPACE and b'workspace too small' in L.rdm_last_error()
    assert m.export(blocks=(MOM[0], MOM[1] - 1) + OBS)[0] == ERR_WORKSPACE and m.export(blocks=MOM + (OBS[0], OBS[1] - 1))[0] == ERR_WORKSPACE
    rc, got, rows = m.export(mom=False, obs=False, outputs=('keys', 'counts', 'sums'))  # the blocks are optional
    assert rc == 0 and rows == 1 and got['keys'].tolist() == [5] and got['counts'].tolist() == [1]
    plain = RawState(64, moments=False, observations=False)  # records that carry moments go into a map without the block with null
    assert plain.add(ok['keys'], ok['counts'], ok['sums']) == (0, 0) and plain.stats()['occupied'] == 1


# ---- the command line ------------------------------------------------------------------------------------------------------------

def tree(tmp_path, name, clouds, poses, seq=5):
    """A dataset root and a directory of pair files whose chain is `poses` relative to poses[0] -> (root, pairs, the chained poses)."""
    from rdmnet_amd import trajectory
    root, pairs = tmp_path / name / 'data', tmp_path / name / 'pairs'
    folder = root / 'downsampled_xyzi' / ('%02d' % seq)
    os.makedirs(folder)
    os.makedirs(pairs)
    frames = [3 * k for k in range(len(clouds))]
    for k, f in enumerate(frames):
        np.save(folder / ('%06d.npy' % f), clouds[k])
    for k in range(len(clouds) - 1):
        T = np.linalg.inv(poses[k + 1]) @ poses[k]
        np.savez(pairs / f'{seq}_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=T, transform=T, information=np.eye(6))
    return root, pairs, trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[seq])[0], frames


def cli(pairs, root, out, *extra):
    from rdmnet_amd import trajectory
    lines = []
    trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(root), '--out', str(out), *extra]),
                   emit=lines.append)
    return lines


def test_trajectory_map_save_and_map_prior_end_to_end(ops, tmp_path):
    """Run 1 fuses the street alone and saves its map; run 2 judges the scans with the car by that prior at 1 m: every car point goes,
    with the restatement's tallies; without the prior the scans' own map keeps car points."""
    from rdmnet_amd import trajectory
    streets, _, scans, poses = scene(5)
    root1, pairs1, X, frames = tree(tmp_path, 'street', streets, poses)
    out1 = tmp_path / 'out1'
    plain = cli(pairs1, root1, tmp_path / 'out0', '--map-voxel', '1', '--map-sharpness')
    lines = cli(pairs1, root1, out1, '--map-voxel', '1', '--map-sharpness', '--map-save')
    assert lines == plain  # --map-save prints nothing
    assert sorted(set(os.listdir(out1)) - set(os.listdir(tmp_path / 'out0'))) == ['5_chained_map_state.npz']
    prior = str(out1 / '5_chained_map_state.npz')
    table = MR.build(streets, X, 1.0, 3)
    saved = ops.read_state(prior)
    same_arrays(saved, dict(SR.export(SR.build(streets, X, 1.0, 3, moments=True)), observations=None), 'the saved state')
    root2, pairs2, X2, _ = tree(tmp_path, 'car', scans, poses)
    assert np.array_equal(X2, X)
    lines = cli(pairs2, root2, tmp_path / 'out2', '--map-voxel', '0.3', '--map-clean', '--map-clean-max-d2', '25', '--map-prior', prior)
    ref = QR.batch(table, None, scans, X, sigma=0.02, max_d2=25.0)
    words = dict(name='5_chained_map_state.npz', voxels=len(table.keys), voxel=1.0, scans=0, moments=True)
    assert lines[-1] == trajectory.clean_line(5, 'chained', ref['tallies'], 1, 25.0, words)
    print(lines[-1])
    assert 'map: ' in lines[-2] and ' at 0.3 m' in lines[-2]  # the scans' own map keeps its own voxel size
    for k, f in enumerate(frames):
        keep = ref['labels'][ref['offsets'][k]:ref['offsets'][k + 1]] == QR.STATIC
        assert np.array_equal(np.load(tmp_path / 'out2' / '5_chained_clean' / ('%06d.npy' % f)), scans[k][keep])
        assert not keep[-CAR:].any() and keep[:-CAR].mean() > 0.9  # every car point goes and the street stays
    own = cli(pairs2, root2, tmp_path / 'out3', '--map-voxel', '1', '--map-clean', '--map-clean-max-d2', '25')
    assert 'judged by' not in own[-1]
    kept_car = 0
    for k, f in enumerate(frames):
        car = {row.tobytes() for row in scans[k][-CAR:]}
        kept_car += sum(row.tobytes() in car for row in np.load(tmp_path / 'out3' / '5_chained_clean' / ('%06d.npy' % f)))
    print(f'own map at 1 m: {kept_car} of {8 * CAR} car points kept')
    assert kept_car > 0


@pytest.mark.parametrize('voxel', [0.3, 1.0])
def test_trajectory_map_localize_end_to_end(ops, tmp_path, voxel):
    """A new drive (another street sample, with the car) from poses 5 cm and 5 mrad off, localised against the saved map of an earlier
    drive under its true poses.  The trajectory's world frame is that of its first chained pose, so the prior is built in that frame."""
    import torch
    from rdmnet_amd import trajectory
    streets, _, _, true = scene(5)
    _, _, drive, _ = scene(6)
    rng = np.random.default_rng(106)
    start = np.stack([perturb(X, rng, 0.05, 0.005) for X in true])
    root, pairs, X, frames = tree(tmp_path, 'drive', drive, start)
    truth = np.linalg.inv(start[0]) @ true
    assert np.abs(X - np.linalg.inv(start[0]) @ start).max() < 1e-12
    prior = gpu_map(ops, streets, truth, voxel, 3, capacity=1 << 16, moments=True)
    path = prior.save(str(tmp_path / 'prior.npz'))
    out = tmp_path / 'out'
    lines = cli(pairs, root, out, '--map-voxel', str(voxel), '--map-localize', '--map-prior', path, '--map-batch', '3')
    paths = [str(root / 'downsampled_xyzi' / '05' / ('%06d.npy' % f)) for f in frames]
    loaded = ops.VoxelMap.load(path)
    localized, stats = trajectory.localize_against_map(paths, X, loaded, batch=3)
    direct = prior.register([dev(c) for c in drive], X)
    assert np.array_equal(localized, direct.transformations.cpu().numpy()) and stats['status'].tolist() == direct.status.tolist() == [1] * 8
    assert stats['iterations'].tolist() == direct.iterations.tolist() and stats['degenerate'] == 0
    written = np.loadtxt(out / '5_localized.txt').reshape(8, 3, 4)
    assert np.abs(written - localized[:, :3]).max() <= 1e-8  # (the file holds nine decimals)
    before = [pose_error(X[k], truth[k])[0] for k in range(8)]
    after = [pose_error(localized[k], truth[k])[0] for k in range(8)]
    print(f'voxel {voxel}: mean translation error {100 * np.mean(before):.2f} -> {100 * np.mean(after):.2f} cm, iterations {stats["iterations"].tolist()}')
    assert np.mean(after) < np.mean(before)
    at = [i for i, s in enumerate(lines) if 'localized' in s]
    assert lines[at[0]].startswith('seq 5 localized: ') and lines[at[1]] == trajectory.localize_line(
        5, stats, dict(name='prior.npz', voxels=len(prior), voxel=voxel, scans=0, moments=True))
    assert lines[at[2]].startswith('seq 5 localized map: ') and sorted(os.listdir(out)) == [
        '5_chained.txt', '5_chained_map.npy', '5_localized.txt', '5_localized_map.npy']
    # five updates, as tests/test_voxel_register_gpu.py caps them, against the restatement on the restated prior
    table = MR.build(streets, truth, voxel, 3)
    five = loaded.register([dev(c) for c in drive], X, max_iteration=5, rot_eps=0.0, trans_eps=0.0).transformations.cpu().numpy()
    worst = 0.0
    for k in range(8):
        want = RR.register(table, drive[k], X[k], 0.02, 4, 1, 5, 0.0, 0.0)
        worst = max(worst, float(np.abs(five[k] - want['transform']).max()))
    print(f'voxel {voxel}: largest pose difference to the restatement after five updates {worst:.3e} (bound {POSE_BOUND:.1e})')
    assert worst <= POSE_BOUND
