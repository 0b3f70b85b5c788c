"""GPU: ops.VoxelMap, the raw rdm_voxel_map_* C-ABI and `python -m rdmnet_amd.trajectory --map-scans` against the NumPy restatement
tests/voxel_map_restatement.py.  Everything is compared with np.array_equal: points, counts, cells, their order and the six counters.
The map is integer sums of fixed-point values, so there is no tolerance anywhere in this file."""
import ctypes
import os

import numpy as np
import pytest

import voxel_map_restatement as VM
from test_voxel_map import FACES, random_pose, with_attribute

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host(res):
    return tuple(t.cpu().numpy() for t in res)


def equal(got, want):
    """(points, counts, cells) bit for bit, dtypes included."""
    for g, w, name in zip(got, want, ('points', 'counts', 'cells')):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        if name == 'points':
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), f'{name}: {int((g != w).sum())} of {g.size} values differ'


def fixture(scans):
    """The three bundled scans with an attribute column under three random rigid poses (any rotation, translations up to 500 m
    of either sign), and the restatement's maps of them: computed once, never changed."""
    if 'clouds' not in _cache:
        rng = np.random.default_rng(11)
        clouds = [with_attribute(scans[k], i) for i, k in enumerate(('s000000', 's000004', 's000007'))]
        poses = np.stack([random_pose(rng) for _ in clouds])
        assert (poses[:, :3, 3] < -50).any() and (poses[:, :3, 3] > 50).any()
        _cache['clouds'] = (clouds, poses, {v: VM.build(clouds, poses, v) for v in (0.3, 0.05)})
    return _cache['clouds']


@pytest.mark.parametrize('voxel', [0.3, 0.05])
def test_scans_under_random_poses(ops, scans, voxel):
    clouds, poses, ref = fixture(scans)
    m = ops.VoxelMap(voxel).integrate([dev(c) for c in clouds], poses)
    want = ref[voxel].extract()
    equal(host(m.extract()), want)
    assert m.stats() == ref[voxel].stats() and len(m) == len(want[0])
    print(f'voxel {voxel}: {sum(len(c) for c in clouds)} points -> {len(want[0])} voxels, at most {want[1].max()} points in one')


def test_one_batch_single_scans_reversed_and_empty_scans_are_one_map(ops, scans):
    import torch
    clouds, poses, ref = fixture(scans)
    want, stats = ref[0.3].extract(), ref[0.3].stats()
    d = [dev(c) for c in clouds]
    empty = torch.zeros((0, 4), dtype=torch.float32, device='cuda')
    forms = {}
    forms['one batch, packed'] = ops.VoxelMap(0.3).integrate(
        (torch.cat(d), torch.tensor([0] + [len(c) for c in clouds], dtype=torch.int64).cumsum(0)), poses)
    single = ops.VoxelMap(0.3)
    for c, X in zip(d, poses):
        single.integrate([c], X)
    forms['one scan per call'] = single
    forms['reversed'] = ops.VoxelMap(0.3).integrate(d[::-1], poses[::-1].copy())
    mixed = ops.VoxelMap(0.3)
    mixed.integrate([d[0], empty, d[1]], np.stack([poses[0], np.eye(4), poses[1]]))
    mixed.integrate([], np.zeros((0, 4, 4)))
    mixed.integrate([empty], [np.eye(4)])
    mixed.integrate([empty, d[2]], torch.from_numpy(np.stack([np.eye(4), poses[2]])))
    forms['with an empty scan and an empty batch'] = mixed
    for name, m in forms.items():
        equal(host(m.extract()), want)
        assert m.stats() == stats, name
    forms['reversed'].reset()
    assert len(forms['reversed']) == 0 and len(forms['reversed'].extract()[0]) == 0
    equal(host(forms['reversed'].integrate(d, poses).extract()), want)  # a reset map is a new map


def special_rows():
    """NaN / inf in a coordinate and in an attribute, points beyond the extent (directly, and through the pose), an attribute >= 2^20
    and one just below, the gate boundaries (r2 == max_range^2: 48, 64, 0 at 80 m; r2 == min_range^2: 3, 4, 0 at 5 m), a point inside
    the minimum range, and ordinary rows."""
    return np.float32([[np.nan, 1, 1, 0.5], [1, np.inf, 1, 0.5], [1, 1, -np.inf, 0.5], [1, 1, 1, np.nan], [1, 1, 1, np.inf],
                       [7, 1, 1, 1048576.0], [7, 1, 1, -1048575.5], [7, 1.1, 1, 1048575.9375], [48, 64, 0, 0.25], [48, 64, 0.01, 0.25],
                       [3, 4, 0, 0.75], [3, 4, -0.01, 0.75], [2.9, 4, 0, 0.1], [-20, -7, 0.25, 0.3], [-20, -7, 0.26, 0.7], [60, 0, 0, 0.2]])


def test_special_rows_faces_and_a_one_point_scan(ops):
    rows = special_rows()
    far = np.eye(4)
    far[0, 3] = 314572.8 - 50.0  # the extent ends at 2^20 cells of 0.3 m: the row at x = 60 leaves it under this pose
    origin = np.zeros((1, 4), np.float32)
    faces = []
    for t in FACES:
        X = np.eye(4)
        X[1, 3] = t
        faces.append(X)
    one = np.float32([[3.0, -4.0, -2.75, 0.125]])
    turn = random_pose(np.random.default_rng(2), 100.0)
    clouds = [rows, rows, one] + [origin] * 4
    poses = np.stack([np.eye(4), far, turn] + faces)
    ref = VM.Map(0.3).integrate(clouds, poses, min_range=0.0, max_range=80.0)
    m = ops.VoxelMap(0.3, capacity=64).integrate([dev(c) for c in clouds], poses, max_range=80.0)
    equal(host(m.extract()), ref.extract())
    st = m.stats()
    assert st == ref.stats() and st['skipped_nonfinite'] == 10 and st['out_of_extent'] >= 3 and st['skipped_range'] == 2
    # the minimum range too, and the faces on their own: y = -0.6, -0.3, 0, 0.3 are the lower faces of cells -2, -1, 0, 1
    ref = VM.Map(0.3).integrate([rows], [np.eye(4)], min_range=5.0, max_range=80.0)
    m = ops.VoxelMap(0.3).integrate([dev(rows)], [np.eye(4)], min_range=5.0, max_range=80.0)
    equal(host(m.extract()), ref.extract())
    assert m.stats() == ref.stats() and m.stats()['skipped_range'] == 2
    pts, counts, cells = host(ops.VoxelMap(0.3).integrate([dev(origin)] * 4, np.stack(faces)).extract())
    assert cells.tolist() == [[0, -2, 0], [0, -1, 0], [0, 0, 0], [0, 1, 0]] and counts.tolist() == [1, 1, 1, 1]
    pts, counts, cells = host(ops.VoxelMap(0.3).integrate([dev(one)], turn).extract())
    equal((pts, counts, cells), VM.build([one], [turn], 0.3).extract())
    assert counts.tolist() == [1]


@pytest.mark.parametrize('voxels', [1, 3])
def test_contention_65536_points_in_few_voxels(ops, voxels):
    rng = np.random.default_rng(voxels)
    n = 65536
    pts = np.concatenate([rng.uniform(0.0, 0.29, (n, 3)), rng.uniform(-1000.0, 1000.0, (n, 1))], 1)
    pts[:, 0] += 0.3 * (np.arange(n) % voxels) - 0.3  # cells -1, 0, 1 along x
    if voxels == 1:
        pts[:, 0] += 0.3
    pts = pts.astype(np.float32)
    X = np.eye(4)
    X[:3, 3] = [-299.7, 150.0, 3.0]
    ref = VM.build([pts], [X], 0.3)
    m = ops.VoxelMap(0.3).integrate([dev(pts)], [X])
    got = host(m.extract())
    equal(got, ref.extract())
    assert len(got[1]) == voxels and got[1].sum() == n and m.stats() == ref.stats()


# ---- the raw C-ABI: a table that is never grown ----------------------------------------------------------------------------

def fmix64(k):
    """The home slot of a key is this (MurmurHash3's 64-bit finaliser) & (capacity - 1): include/rdmnet_hip.h."""
    m = (1 << 64) - 1
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & m
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & m
    k ^= k >> 33
    return k


def key_of(cell):
    return ((cell[0] + VM.HALF) << 42) | ((cell[1] + VM.HALF) << 21) | (cell[2] + VM.HALF)


class RawMap:
    def __init__(self, capacity, channels, voxel):
        import torch
        from rdmnet_amd import _lib
        self.L, self._lib, self.torch = _lib.lib(), _lib, torch
        self.capacity, self.channels, self.voxel = capacity, channels, voxel
        nbytes = self.L.rdm_voxel_map_bytes(capacity, channels)
        assert nbytes >= 6 * 8 + capacity * (12 + 8 * channels)
        self.buf = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
        self.head = (self.buf.data_ptr(), nbytes, capacity, channels)
        assert self.L.rdm_voxel_map_reset(*self.head, _lib.stream_ptr()) == 0

    def integrate(self, clouds, poses, lo=0.0, hi=float('inf')):
        pts = dev(np.concatenate(clouds))
        off = dev(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), np.int64)
        X = dev(np.asarray(poses, np.float64).reshape(-1, 16), np.float64)
        return self.L.rdm_voxel_map_integrate(*self.head, self.voxel, pts.data_ptr(), pts.shape[1], pts.shape[0], off.data_ptr(),
                                              X.data_ptr(), len(clouds), lo, hi, self._lib.stream_ptr())

    def stats(self):
        out = (ctypes.c_uint64 * 6)()
        assert self.L.rdm_voxel_map_stats(*self.head, ctypes.addressof(out), self._lib.stream_ptr()) == 0
        return dict(zip(VM.STATS, (int(v) for v in out)))

    def extract(self, min_points=1):
        torch, S, C = self.torch, self.capacity, self.channels
        pts = torch.empty((S, C), dtype=torch.float32, device='cuda')
        counts = torch.empty((S,), dtype=torch.int32, device='cuda')
        cells = torch.empty((S, 3), dtype=torch.int32, device='cuda')
        n = torch.zeros((1,), dtype=torch.int64, device='cuda')
        ws = torch.empty((self.L.rdm_voxel_map_extract_workspace_bytes(S),), dtype=torch.uint8, device='cuda')
        assert self.L.rdm_voxel_map_extract(*self.head, self.voxel, min_points, pts.data_ptr(), counts.data_ptr(), cells.data_ptr(), S,
                                            n.data_ptr(), ws.data_ptr(), ws.numel(), self._lib.stream_ptr()) == 0
        m = int(n.item())
        return host((pts[:m], counts[:m], cells[:m]))


def clustered_cells(n, capacity, first_home):
    """n distinct cells (some with negative indices) whose home slots all lie in [first_home, capacity)."""
    out = []
    for i in range(-40, 40):
        for j in range(-40, 40):
            if fmix64(key_of((i, j, 2))) & (capacity - 1) >= first_home:
                out.append((i, j, 2))
    assert len(out) >= n
    return np.array(out[:n], np.int64)


def points_in_cells(cells, per_cell, voxel, rng):
    c = np.repeat(cells, per_cell, axis=0).astype(np.float64)
    xyz = (c + rng.uniform(0.1, 0.9, c.shape)) * voxel
    pts = np.concatenate([xyz, rng.uniform(-5.0, 5.0, (len(c), 1))], 1).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def test_raw_abi_collisions_long_probes_and_wrap_around():
    """40 voxels whose home slots are the last 8 of a 64-slot table: probe sequences of up to 40 slots that wrap at the table's end."""
    rng = np.random.default_rng(5)
    cells = clustered_cells(40, 64, 56)
    pts = points_in_cells(cells, 50, 0.5, rng)
    ref = VM.build([pts[:1000], pts[1000:]], [np.eye(4), np.eye(4)], 0.5)
    assert len(ref.keys) == 40
    m = RawMap(64, 4, 0.5)
    assert m.integrate([pts[:1000], pts[1000:]], [np.eye(4), np.eye(4)]) == 0
    equal(m.extract(), ref.extract())
    assert m.stats() == ref.stats()
    # into a larger table and back into one of the same size: the same map, the counters carried over
    big = RawMap(256, 4, 0.5)
    assert m.L.rdm_voxel_map_rehash(*m.head[:3], *big.head[:3], 4, m._lib.stream_ptr()) == 0
    equal(big.extract(), ref.extract())
    assert big.stats() == ref.stats()
    assert big.L.rdm_voxel_map_rehash(*big.head[:3], *m.head[:3], 4, m._lib.stream_ptr()) != 0  # (a smaller table is refused)
    equal(m.extract(min_points=51), ref.extract(min_points=51))
    assert len(m.extract(min_points=50)[0]) == 40


def test_raw_abi_table_full_drops_whole_keys_and_ends():
    """200 distinct voxels into 64 slots: the call returns RDM_OK (the probe is bounded), the table is full, every stored voxel is
    the restatement's voxel of that key exactly, and the dropped points are counted."""
    rng = np.random.default_rng(6)
    cells = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-2, 3), np.arange(4), indexing='ij'), -1).reshape(-1, 3)
    assert len(cells) == 200
    pts = points_in_cells(cells, 20, 0.3, rng)
    pts[7, 0] = np.nan  # one skipped row: kept points = rows - 1
    ref = VM.build([pts], [np.eye(4)], 0.3)
    assert len(ref.keys) == 200
    m = RawMap(64, 4, 0.3)
    assert m.integrate([pts], [np.eye(4)]) == 0
    got = m.extract()
    st = m.stats()
    assert st['occupied'] == 64 and len(got[1]) == 64
    assert (np.diff([key_of(tuple(int(v) for v in c)) for c in got[2]]) > 0).all()  # ascending keys
    equal(got, ref.subset(got[2]))  # all or nothing per key
    kept = len(pts) - 1
    assert st['skipped_nonfinite'] == 1 and st['integrated'] == int(got[1].sum()) and st['dropped_full'] == kept - int(got[1].sum())
    # a second batch of the same points: the stored keys double, nothing else gets in
    assert m.integrate([pts], [np.eye(4)]) == 0
    again = m.extract()
    assert np.array_equal(again[2], got[2]) and np.array_equal(again[1], 2 * got[1])
    assert m.stats()['dropped_full'] == 2 * st['dropped_full']


def test_growth_equals_a_map_created_large_enough(ops, scans):
    clouds, poses, ref = fixture(scans)
    small = ops.VoxelMap(0.3, capacity=1024)
    seen = {small.capacity}
    for c, X in zip(clouds, poses):
        for part in np.array_split(c, 4):
            small.integrate([dev(part)], [X])
            seen.add(small.capacity)
    large = ops.VoxelMap(0.3, capacity=1 << 18).integrate([dev(c) for c in clouds], poses)
    assert len(seen) >= 4 and large.capacity == 1 << 18, sorted(seen)
    a, b = host(small.extract()), host(large.extract())
    equal(a, b)
    equal(a, ref[0.3].extract())
    assert small.stats() == large.stats() == ref[0.3].stats() and small.stats()['dropped_full'] == 0


def test_extract_min_points_is_the_matching_subset(ops, scans):
    clouds, poses, ref = fixture(scans)
    m = ops.VoxelMap(0.3).integrate([dev(c) for c in clouds], poses)
    pts, counts, cells = host(m.extract())
    sub = host(m.extract(min_points=3))
    keep = counts >= 3
    assert 0 < keep.sum() < len(keep)
    equal(sub, (pts[keep], counts[keep], cells[keep]))
    equal(sub, ref[0.3].extract(min_points=3))


def test_three_channels_from_a_strided_input(ops, scans):
    clouds, poses, _ = fixture(scans)
    wide = dev(np.concatenate([clouds[0], clouds[0][:, :2]], 1))  # ld = 6
    m = ops.VoxelMap(0.3, channels=3).integrate([wide[:, :3]], poses[:1])
    assert wide[:, :3].stride(0) == 6
    ref = VM.build([clouds[0][:, :3]], poses[:1], 0.3, channels=3)
    equal(host(m.extract()), ref.extract())
    assert m.stats() == ref.stats()
    m8 = ops.VoxelMap(0.3, channels=6).integrate([wide], poses[:1])
    equal(host(m8.extract()), VM.build([wide.cpu().numpy()], poses[:1], 0.3, channels=6).extract())


def test_arguments_are_rejected_by_name(ops, scans):
    import torch
    clouds, poses, _ = fixture(scans)
    m = ops.VoxelMap(0.3)
    c = dev(clouds[0][:100])
    for bad, match in ((lambda: ops.VoxelMap(0.0), 'voxel'), (lambda: ops.VoxelMap(0.3, channels=9), 'channels'),
                       (lambda: ops.VoxelMap(0.3, capacity=1000), 'capacity'), (lambda: ops.VoxelMap(0.3, device='cpu'), 'CUDA'),
                       (lambda: m.integrate([c.double()], poses[:1]), r'clouds\[0\]'), (lambda: m.integrate([c[:, :3]], poses[:1]), r'clouds\[0\]'),
                       (lambda: m.integrate([c, c.cpu()], poses[:2]), r'clouds\[1\]'), (lambda: m.integrate([c], np.eye(3)[None]), 'poses'),
                       (lambda: m.integrate([c], poses[:2]), 'poses'), (lambda: m.integrate([c], [np.full((4, 4), np.nan)]), 'finite'),
                       (lambda: m.integrate([c], poses[:1], min_range=9.0, max_range=3.0), 'min_range'),
                       (lambda: m.integrate((c, torch.zeros((2, 2), dtype=torch.int64)), poses[:1]), 'offsets'),
                       (lambda: m.integrate(c, poses[:1]), 'clouds')):
        with pytest.raises(ValueError, match=match):
            bad()
    assert len(m) == 0


# ---- the command line ------------------------------------------------------------------------------------------------------

def test_trajectory_map_scans_end_to_end(ops, scans, tmp_path):
    """Three frames: one scan seen from the identity and from two known poses.  The map written by the command line equals build_map
    on the same inputs, and a middle pose that is off by 1 m gives strictly more voxels than the true poses."""
    from rdmnet_amd import trajectory
    rng = np.random.default_rng(9)
    world = with_attribute(scans['s000000'], 3)
    X = [np.eye(4), random_pose(rng, 3.0), random_pose(rng, 6.0)]
    data = tmp_path / 'data'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    frames = [0, 4, 9]
    for f, Xk in zip(frames, X):
        inv = np.linalg.inv(Xk)
        local = world.copy()
        local[:, :3] = (world[:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        np.save(folder / ('%06d.npy' % f), local)
    T = [np.linalg.inv(X[k + 1]) @ X[k] for k in range(2)]  # X_ref = X_src inv(T)

    def run(name, transforms, extra=()):
        pairs, out = tmp_path / f'pairs_{name}', tmp_path / f'out_{name}'
        pairs.mkdir()
        for k in range(2):
            np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=transforms[k], transform=T[k], information=np.eye(6))
        lines = []
        args = trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                    '--map-batch', '2', *extra])
        trajectory.run(args, emit=lines.append)
        line = [s for s in lines if ' map: ' in s]
        assert len(line) == (2 if '--optimize' in extra else 1) and line[0].startswith('seq 5 chained map: '), lines
        assert all(' voxels at 0.3 m, ' in s for s in line)
        if '--optimize' in extra:
            assert line[1].startswith('seq 5 optimized map: ')
            _cache['optimized'] = (np.load(out / '5_optimized_map.npy'), np.loadtxt(str(out / '5_optimized.txt')).reshape(-1, 3, 4))
        nodes = trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0]
        return np.load(out / '5_chained_map.npy'), int(line[0].split(' map: ')[1].split(' voxels')[0]), nodes, line[0]

    written, voxels, nodes, line = run('true', T)
    assert written.dtype == np.float32 and written.shape == (voxels, 5)
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    vmap = trajectory.build_map(paths, nodes)
    pts, counts, _ = host(vmap.extract())
    assert np.array_equal(written[:, :4].view(np.uint32), pts.view(np.uint32)) and np.array_equal(written[:, 4], counts.astype(np.float32))
    clouds = [np.load(p) for p in paths]
    equal(host(vmap.extract()), VM.build(clouds, nodes, 0.3).extract())
    assert f'{3 * len(world)} points' in line and int(counts.sum()) == 3 * len(world)
    off = np.eye(4)
    off[0, 3] = 1.0
    _, worse, _, _ = run('off', [off @ T[0], T[1] @ np.linalg.inv(off)])  # the middle pose moves by 1 m, the last one stays
    print(f'true poses: {voxels} voxels; middle pose off by 1 m: {worse} voxels; one scan alone: {len(VM.build(clouds[:1], nodes[:1], 0.3).keys)}')
    assert worse > voxels
    # --optimize: the optimised poses get a map of their own
    run('optimize', T, ['--optimize'])
    opt_map, opt_poses = _cache.pop('optimized')
    nodes_opt = np.tile(np.eye(4), (3, 1, 1))
    nodes_opt[:, :3] = opt_poses
    assert np.abs(nodes_opt - nodes).max() < 1e-6  # (exact pairs, no loops: nothing to optimise; the file has 10 digits)
    assert opt_map.shape[1] == 5 and int(opt_map[:, 4].sum()) == 3 * len(world) and worse > len(opt_map)
    sub, n_sub, _, _ = run('min3', T, ['--map-min-points', '3', '--map-range', '2', '40'])
    assert n_sub < voxels and sub.shape == (n_sub, 5) and (sub[:, 4] >= 3).all()
