"""GPU: the voxel moments (ops.VoxelMap(moments=True), the raw rdm_voxel_moments_* / rdm_voxel_map_*_moments C-ABI and `python -m
rdmnet_amd.trajectory --map-sharpness`) against the NumPy restatement tests/voxel_moments_restatement.py.

The nine sums are integer sums and the covariance is float64 with the restatement's association, so both are compared with
np.array_equal (the covariance on its bits).  The eigenvalues are compared with numpy.linalg.eigvalsh of the SAME float64 matrix
within 1e-12 ||cov||_F: the backward error of Jacobi is a few eps ||cov|| and Weyl's theorem carries that bound to the
eigenvalues, so the bound is three to four orders above the solver's error and far below the effect of any wrong entry.  The
normals are compared where the gap l1 - l0 is at least 1e-3 ||cov||_F, with |sin(angle)| <= 1e-9 (Davis-Kahan: the eigenvalue
bound over the gap)."""
import os
import re

import numpy as np
import pytest

import voxel_map_restatement as VM
import voxel_moments_restatement as MR
from test_voxel_map import FACES, random_pose, with_attribute
from test_voxel_map_gpu import RawMap, dev, equal, host, points_in_cells, special_rows

pytestmark = pytest.mark.gpu

_cache = {}
NAMES = ('sums', 'cov', 'eigenvalues', 'normals')


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def fixture(scans):
    """The 300 points nearest to the sensor of each bundled scan (dense: several points a voxel) with an attribute column, under three
    random rigid poses, and the restatement's moments of them at 0.3 m and 1 m: computed once, never changed."""
    if 'clouds' not in _cache:
        rng = np.random.default_rng(21)
        clouds = []
        for i, k in enumerate(('s000000', 's000004', 's000007')):
            c = scans[k]
            clouds.append(with_attribute(c[np.argsort(np.linalg.norm(c[:, :2], axis=1), kind='stable')[:300 + i]], i))
        poses = np.stack([random_pose(rng) for _ in clouds])
        _cache['clouds'] = (clouds, poses, {v: MR.build(clouds, poses, v) for v in (0.3, 1.0)})
    return _cache['clouds']


def moments_equal(got, want, what=''):
    """sums and cov bit for bit, dtypes and shapes included."""
    for g, w, name in zip(got[:2], want[:2], NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        g, w = (g.view(np.uint64), w.view(np.uint64)) if name == 'cov' else (g, w)
        assert np.array_equal(g, w), f'{what} {name}: {int((g != w).sum())} of {g.size} values differ'


def same_bytes(a, b, what=''):
    for g, w, name in zip(a, b, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)


def check_eigen(cov, w, normals):
    """The solver's outputs against numpy on the same matrices -> (max eigenvalue error / ||cov||_F, max |sin| over the rows with a gap,
    the number of such rows)."""
    A = MR.full(cov)
    fro = np.sqrt((A * A).sum((1, 2)))
    want, vec = np.linalg.eigh(A)
    assert w.dtype == np.float64 and w.shape == want.shape and normals.shape == want.shape
    assert (np.diff(w, axis=1) >= 0).all()  # ascending
    err = np.abs(w - want).max(1)
    assert (err <= 1e-12 * fro).all(), f'eigenvalues: {(err / np.maximum(fro, 1e-300)).max():.3e} ||cov||_F'
    assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-15  # (a few roundings: the division by the length, and this norm)
    assert np.array_equal(MR.signed(normals), normals)  # the sign rule, on the output itself
    gap = (want[:, 1] - want[:, 0]) >= 1e-3 * fro
    gap &= fro > 0
    v0 = MR.signed(vec[:, :, 0])
    sin = np.linalg.norm(np.cross(normals, v0), axis=1)
    assert (sin[gap] <= 1e-9).all(), f'normals: |sin| up to {sin[gap].max():.3e}'
    # where the largest component is not tied with another one, the sign rule gives numpy's signed vector itself
    top = np.sort(np.abs(v0), axis=1)
    clear = gap & (top[:, 2] - top[:, 1] > 1e-6)
    assert ((normals[clear] * v0[clear]).sum(1) > 0).all()
    rel = float((err[fro > 0] / fro[fro > 0]).max()) if (fro > 0).any() else 0.0
    return rel, float(sin[gap].max()) if gap.any() else 0.0, int(gap.sum())


@pytest.mark.parametrize('voxel', [0.3, 1.0])
def test_scans_under_random_poses(ops, scans, voxel):
    clouds, poses, ref = fixture(scans)
    m = ops.VoxelMap(voxel, capacity=4096, moments=True).integrate([dev(c) for c in clouds], poses)
    got, want = host(m.extract_moments()), ref[voxel].extract()
    moments_equal(got, want)
    assert m.stats() == ref[voxel].map.stats() and m.capacity == 4096
    equal(host(m.extract()), ref[voxel].map.extract())
    rel, sin, rows = check_eigen(*got[1:])
    counts = ref[voxel].map.counts
    print(f'voxel {voxel}: {int(counts.sum())} points -> {len(counts)} voxels, at most {counts.max()} points in one; eigenvalue error '
          f'{rel:.2e} ||cov||_F, |sin| of the normals {sin:.2e} over {rows} voxels with a gap')
    # min_points selects the matching rows
    sub, keep = host(m.extract_moments(min_points=4)), counts >= 4
    assert 0 < keep.sum() < len(keep)
    same_bytes(sub, tuple(g[keep] for g in got))


def test_the_base_map_is_unchanged_by_the_moments(ops, scans):
    clouds, poses, ref = fixture(scans)
    d = [dev(c) for c in clouds]
    plain = ops.VoxelMap(0.3, capacity=4096).integrate(d, poses)
    with_moments = ops.VoxelMap(0.3, capacity=4096, moments=True).integrate(d, poses)
    assert plain._mom is None and with_moments._mom is not None
    equal(host(with_moments.extract()), host(plain.extract()))
    equal(host(with_moments.extract(3)), host(plain.extract(3)))
    assert with_moments.stats() == plain.stats()
    assert with_moments._buf.numel() == plain._buf.numel()


def test_one_batch_single_scans_reversed_and_empty_scans_are_one_map(ops, scans):
    import torch
    clouds, poses, ref = fixture(scans)
    want, stats = ref[0.3].extract(), ref[0.3].map.stats()
    d = [dev(c) for c in clouds]
    empty = torch.zeros((0, 4), dtype=torch.float32, device='cuda')
    new = lambda: ops.VoxelMap(0.3, capacity=4096, moments=True)
    forms = {}
    forms['one batch, packed'] = new().integrate((torch.cat(d), torch.tensor([0] + [len(c) for c in clouds], dtype=torch.int64).cumsum(0)), poses)
    single = new()
    for c, X in zip(d, poses):
        single.integrate([c], X)
    forms['one scan per call'] = single
    forms['reversed'] = new().integrate(d[::-1], poses[::-1].copy())
    mixed = new()
    mixed.integrate([d[0], empty, d[1]], np.stack([poses[0], np.eye(4), poses[1]]))
    mixed.integrate([], np.zeros((0, 4, 4)))
    mixed.integrate([empty, d[2]], np.stack([np.eye(4), poses[2]]))
    forms['with an empty scan and an empty batch'] = mixed
    first = None
    for name, m in forms.items():
        got = host(m.extract_moments())
        moments_equal(got, want, name)
        assert m.stats() == stats, name
        first = first or got
        same_bytes(got, first, name)  # the eigenvalues and the normals too
    forms['reversed'].reset()
    assert len(forms['reversed']) == 0 and all(len(t) == 0 for t in forms['reversed'].extract_moments())
    same_bytes(host(forms['reversed'].integrate(d, poses).extract_moments()), first, 'after reset')  # a reset map is a new map


@pytest.mark.parametrize('voxels', [1, 4])
def test_contention_65536_points_in_few_voxels(ops, voxels):
    rng = np.random.default_rng(voxels)
    n = 65536
    pts = rng.uniform(0.0, 0.29, (n, 3))
    pts[:, 0] += 0.3 * (np.arange(n) % voxels) - 0.6  # cells -2 ... 1 along x (or -2 alone)
    pts = pts.astype(np.float32)
    X = np.eye(4)
    X[:3, 3] = [-299.7, 150.0, 3.0]
    ref = MR.build([pts], [X], 0.3, channels=3)
    m = ops.VoxelMap(0.3, channels=3, capacity=1 << 17, moments=True).integrate([dev(pts)], [X])
    got = host(m.extract_moments())
    moments_equal(got, ref.extract())
    assert m.capacity == 1 << 17 and len(got[0]) == voxels and m.stats() == ref.map.stats()
    assert got[0][:, 3].max() > 2 ** 31  # sums beyond 32 bits
    check_eigen(*got[1:])


def test_growth_equals_a_map_created_large_enough(ops, scans):
    clouds, poses, ref = fixture(scans)
    small = ops.VoxelMap(0.3, capacity=64, moments=True)
    seen = {small.capacity}
    for c, X in zip(clouds, poses):
        for part in np.array_split(c, 12):
            small.integrate([dev(part)], [X])
            seen.add(small.capacity)
    large = ops.VoxelMap(0.3, capacity=4096, moments=True).integrate([dev(c) for c in clouds], poses)
    assert len(seen) >= 4 and large.capacity == 4096, sorted(seen)
    a, b = host(small.extract_moments()), host(large.extract_moments())
    same_bytes(a, b)
    moments_equal(a, ref[0.3].extract())
    equal(host(small.extract()), ref[0.3].map.extract())
    assert small.stats() == large.stats() == ref[0.3].map.stats() and small.stats()['dropped_full'] == 0


def test_special_rows_faces_and_negative_cells(ops):
    rows = special_rows()
    far = np.eye(4)
    far[0, 3] = 314572.8 - 50.0  # the row at x = 60 leaves the extent under this pose
    origin = np.zeros((1, 4), np.float32)
    faces = []
    for t in FACES:
        X = np.eye(4)
        X[1, 3] = t
        faces.append(X)
    # u = 0 and u = 4095 on both sides of zero, at 0.25 m voxels through the rows themselves (exact in float32)
    step = 2.0 ** -14
    edge = np.float32([[0.25, -0.25, 0.0, 0.5], [0.25 - step, -0.25 - step, -step, 0.5], [-0.5, -0.5 + 4095 * step, 0.25 + 4095 * step, 0.1]])
    turn = random_pose(np.random.default_rng(2), 100.0)
    clouds = [rows, rows, rows[::-1].copy()] + [origin] * 4
    poses = np.stack([np.eye(4), far, turn] + faces)
    ref = MR.Moments(0.3).integrate(clouds, poses, min_range=0.0, max_range=80.0)
    m = ops.VoxelMap(0.3, capacity=64, moments=True).integrate([dev(c) for c in clouds], poses, max_range=80.0)
    got = host(m.extract_moments())
    moments_equal(got, ref.extract())
    st = m.stats()
    assert st == ref.map.stats() and st['skipped_nonfinite'] == 15 and st['out_of_extent'] >= 3 and st['skipped_range'] == 3
    assert int(got[0][:, :3].min()) >= 0 and int(got[0][:, :3].max()) < 4096 * int(ref.map.counts.max())
    check_eigen(*got[1:])
    # the minimum range too
    ref = MR.Moments(0.3).integrate([rows], [np.eye(4)], min_range=5.0, max_range=80.0)
    m = ops.VoxelMap(0.3, moments=True, capacity=64).integrate([dev(rows)], [np.eye(4)], min_range=5.0, max_range=80.0)
    moments_equal(host(m.extract_moments()), ref.extract())
    assert m.stats() == ref.map.stats() and m.stats()['skipped_range'] == 2
    ref = MR.build([edge], [np.eye(4)], 0.25)
    m = ops.VoxelMap(0.25, moments=True, capacity=64).integrate([dev(edge)], [np.eye(4)])
    sums, cov, w, normal = host(m.extract_moments())
    moments_equal((sums, cov), ref.extract())
    _, _, cells = host(m.extract())
    assert cells.tolist() == [[-2, -2, 1], [0, -2, -1], [1, -1, 0]]
    assert sums[:, :3].tolist() == [[0, 4095, 4095], [4095, 4095, 4095], [0, 0, 0]] and (cov == 0).all() and (w == 0).all()


# ---- the raw C-ABI -------------------------------------------------------------------------------------------------------------

class RawMoments(RawMap):
    """A table that is never grown, with its moments block beside it."""

    def __init__(self, capacity, channels, voxel):
        super().__init__(capacity, channels, voxel)
        nbytes = self.L.rdm_voxel_moments_bytes(capacity)
        assert nbytes >= 72 * capacity
        self.mom = self.torch.empty((nbytes,), dtype=self.torch.uint8, device='cuda')
        assert self.L.rdm_voxel_moments_reset(self.mom.data_ptr(), nbytes, capacity, self._lib.stream_ptr()) == 0

    def integrate_moments(self, clouds, poses, lo=0.0, hi=float('inf'), short=0):
        pts = dev(np.concatenate(clouds))
        off = dev(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), np.int64)
        X = dev(np.asarray(poses, np.float64).reshape(-1, 16), np.float64)
        return self.L.rdm_voxel_map_integrate_moments(*self.head, self.voxel, pts.data_ptr(), pts.shape[1], pts.shape[0], off.data_ptr(),
                                                      X.data_ptr(), len(clouds), lo, hi, self.mom.data_ptr(), self.mom.numel() - short,
                                                      self._lib.stream_ptr())

    def extract_moments(self, min_points=1, short=0, with_sums=True):
        torch, S = self.torch, self.capacity
        sums = torch.empty((S, 9), dtype=torch.int64, device='cuda')
        cov = torch.empty((S, 6), dtype=torch.float64, device='cuda')
        eig = torch.empty((S, 3), dtype=torch.float64, device='cuda')
        normals = torch.empty((S, 3), dtype=torch.float64, device='cuda')
        n = torch.zeros((1,), dtype=torch.int64, device='cuda')
        ws = torch.empty((self.L.rdm_voxel_map_extract_workspace_bytes(S),), dtype=torch.uint8, device='cuda')
        rc = self.L.rdm_voxel_map_extract_moments(*self.head, self.mom.data_ptr(), self.mom.numel() - short, self.voxel, min_points,
                                                  sums.data_ptr() if with_sums else 0, cov.data_ptr(), eig.data_ptr(), normals.data_ptr(),
                                                  S, n.data_ptr(), ws.data_ptr(), ws.numel(), self._lib.stream_ptr())
        if rc != 0:
            return rc
        m = int(n.item())
        return host((sums[:m], cov[:m], eig[:m], normals[:m]))


def test_raw_abi_a_moments_block_that_is_too_small_is_refused():
    ERR_WORKSPACE = -2  # RDM_ERR_WORKSPACE
    rng = np.random.default_rng(3)
    pts = points_in_cells(np.array([[0, 0, 0], [-1, 2, 0]]), 10, 0.5, rng)
    m = RawMoments(64, 4, 0.5)
    assert m.L.rdm_voxel_moments_bytes(63) == 0 and m.L.rdm_voxel_moments_bytes(64) == 64 * 72
    assert m.integrate_moments([pts], [np.eye(4)], short=1) == ERR_WORKSPACE
    assert b'moments block is too small' in m.L.rdm_last_error()
    assert m.stats()['integrated'] == 0  # nothing ran
    assert m.extract_moments(short=8) == ERR_WORKSPACE
    assert m.L.rdm_voxel_moments_reset(m.mom.data_ptr(), m.mom.numel() - 1, 64, m._lib.stream_ptr()) == ERR_WORKSPACE
    big = RawMoments(128, 4, 0.5)
    args = (*m.head[:3], m.mom.data_ptr(), m.mom.numel(), *big.head[:3], big.mom.data_ptr())
    assert m.L.rdm_voxel_moments_rehash(*args, big.mom.numel() - 1, 4, m._lib.stream_ptr()) == ERR_WORKSPACE
    # the same calls with whole blocks: the map, its rehash into 128 slots, and the sums without the optional output
    assert m.integrate_moments([pts], [np.eye(4)]) == 0
    ref = MR.build([pts], [np.eye(4)], 0.5)
    moments_equal(m.extract_moments(), ref.extract())
    assert m.L.rdm_voxel_map_rehash(*m.head[:3], *big.head[:3], 4, m._lib.stream_ptr()) == 0
    assert m.L.rdm_voxel_moments_rehash(*args, big.mom.numel(), 4, m._lib.stream_ptr()) == 0
    moments_equal(big.extract_moments(), ref.extract())
    same_bytes(big.extract_moments(with_sums=False)[1:], m.extract_moments()[1:])
    assert big.integrate_moments([pts], [np.eye(4)]) == 0  # the slots the rehash did not fill are zero: new keys start from nothing
    other = points_in_cells(np.array([[5, 5, 5], [-7, 0, 1], [0, 0, 1]]), 7, 0.5, rng)
    assert big.integrate_moments([other], [np.eye(4)]) == 0
    moments_equal(big.extract_moments(), MR.build([pts, pts, other], [np.eye(4)] * 3, 0.5).extract())


def test_raw_abi_table_full_drops_whole_keys_and_ends():
    """200 distinct voxels into 64 slots, sized as test_voxel_map_gpu's test of the same name: the call returns RDM_OK by the bounded
    probe, and what the table stores for a key is the restatement's voxel of that key, moments included."""
    rng = np.random.default_rng(6)
    cells = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-2, 3), np.arange(4), indexing='ij'), -1).reshape(-1, 3)
    pts = points_in_cells(cells, 20, 0.3, rng)
    pts[7, 0] = np.nan
    ref = MR.build([pts], [np.eye(4)], 0.3)
    assert len(ref.keys) == 200
    m = RawMoments(64, 4, 0.3)
    assert m.integrate_moments([pts], [np.eye(4)]) == 0
    got, mom, st = m.extract(), m.extract_moments(), m.stats()
    assert st['occupied'] == 64 and len(got[1]) == 64 and st['dropped_full'] > 0
    equal(got, ref.map.subset(got[2]))
    moments_equal(mom, ref.subset(got[2]))
    assert st['integrated'] == int(got[1].sum()) and st['dropped_full'] == len(pts) - 1 - int(got[1].sum())
    assert int(mom[0][:, :3].sum()) <= 4095 * 3 * st['integrated']  # (a dropped point added nothing)
    assert m.integrate_moments([pts], [np.eye(4)]) == 0
    again = m.extract_moments()
    assert np.array_equal(again[0], 2 * mom[0]) and m.stats()['dropped_full'] == 2 * st['dropped_full']


# ---- the eigen-solver on constructed voxels ------------------------------------------------------------------------------------

def constructed_voxels():
    """1 m voxels, one shape per cell along x (cells -2 ... 3); coordinates are cell + u / 4096 (exact in float32) unless said."""
    rng = np.random.default_rng(8)
    n = np.array([1.0, 2.0, 2.0]) / 3.0
    t1, t2 = np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0), np.cross(n, np.array([2.0, -1.0, 0.0]) / np.sqrt(5.0))
    ab = rng.uniform(-0.3, 0.3, (200, 2))
    shapes = {
        'tilted plane': 0.5 + ab[:, :1] * t1 + ab[:, 1:] * t2,                                  # normal (1, 2, 2) / 3, quantised
        'line': 0.1 + np.linspace(0.0, 0.8, 50)[:, None] * np.array([[0.6, 0.0, 0.8]]),
        'blob': rng.uniform(0.05, 0.95, (300, 3)),
        'single point': np.array([[0.3, 0.7, 0.123]]),
        'coplanar': np.array([[4050 - 2 * (b + c), b, c] for b in range(0, 1001, 200) for c in range(0, 1001, 200)]) / 4096.0,
        'thin slab': np.concatenate([rng.uniform(0.1, 0.9, (100, 2)), 0.5 + rng.normal(0.0, 0.004, (100, 1))], 1),
    }
    clouds, order = [], []
    for cell, (name, p) in zip(range(-2, 4), shapes.items()):
        assert p.min() >= 0 and p.max() < 1
        q = p.copy()
        q[:, 0] += cell
        clouds.append(q.astype(np.float32))
        order.append(name)
    return order, clouds


def test_eigen_solver_on_constructed_voxels(ops):
    order, clouds = constructed_voxels()
    poses = np.tile(np.eye(4), (len(clouds), 1, 1))
    ref = MR.build(clouds, poses, 1.0, channels=3)
    m = ops.VoxelMap(1.0, channels=3, capacity=64, moments=True).integrate([dev(c) for c in clouds], poses)
    sums, cov, w, normal = host(m.extract_moments())
    moments_equal((sums, cov), ref.extract())
    assert len(w) == len(order)  # one voxel per shape, in cell order
    rel, sin, rows = check_eigen(cov, w, normal)
    print(f'constructed voxels: eigenvalue error {rel:.2e} ||cov||_F, |sin| {sin:.2e} over {rows} voxels with a gap')
    row = dict(zip(order, range(len(order))))
    n = np.array([1.0, 2.0, 2.0]) / 3.0
    for name in ('tilted plane', 'coplanar'):
        assert np.linalg.norm(np.cross(normal[row[name]], n)) < 2e-3 and normal[row[name]] @ n > 0, name
    assert np.linalg.norm(np.cross(normal[row['coplanar']], n)) < 1e-9
    assert abs(w[row['coplanar'], 0]) <= 1e-12 * np.linalg.norm(MR.full(cov)[row['coplanar']])  # flat: zero up to the bound
    assert w[row['tilted plane'], 0] < (1.0 / 4096) ** 2 and w[row['tilted plane'], 1] > 1e-3  # as thick as the quantisation
    assert (w[row['line'], :2] < 1e-7).all() and w[row['line'], 2] > 0.05
    assert 0.6 < w[row['blob'], 0] / w[row['blob'], 2] <= 1.0 and abs(w[row['blob'], 1] - 0.9 ** 2 / 12) < 0.02
    assert (cov[row['single point']] == 0).all() and (w[row['single point']] == 0).all()
    assert abs(np.sqrt(w[row['thin slab'], 0]) - 0.004) < 0.001 and abs(normal[row['thin slab'], 2]) > 0.999 and normal[row['thin slab'], 2] > 0


# ---- the report ----------------------------------------------------------------------------------------------------------------

def test_sharpness_agrees_with_the_restatement(ops, scans):
    clouds, poses, _ = fixture(scans)
    # beside the scans: voxels of 4, 5 and 3 identical points far away (zero covariance: degenerate) and one of 2
    same = [np.repeat(np.float32([[900.0 + 3 * k, -4.0, 2.0, 0.5]]), n, axis=0) for k, n in enumerate((4, 5, 3, 2))]
    clouds, poses = list(clouds) + same, np.concatenate([poses, np.tile(np.eye(4), (4, 1, 1))])
    ref = MR.build(clouds, poses, 1.0)
    m = ops.VoxelMap(1.0, capacity=4096, moments=True).integrate([dev(c) for c in clouds], poses)
    for min_points, degenerate in ((4, 2), (5, 1), (3, None)):
        want = ref.sharpness(min_points)
        # the comparison of `degenerate` is well posed: every qualified voxel is either exactly zero or clearly of full rank
        _, cov, w, _ = ref.extract(min_points)
        fro = np.linalg.norm(MR.full(cov), axis=(1, 2))
        posed = ((cov == 0).all(1) & (w[:, 0] == 0)) | (w[:, 0] > 1e-9 * fro)
        if degenerate is None:
            assert not posed.all()  # (three points are coplanar: l0 is zero up to rounding, of either sign)
        else:
            assert posed.all() and want['degenerate'] == degenerate
        got = m.sharpness(min_points)
        print(min_points, got)
        assert set(got) == {'voxels', 'qualified', 'degenerate', 'plane_thickness', 'entropy'}
        assert got['voxels'] == want['voxels'] == len(ref.keys) and got['qualified'] == want['qualified'] == int((ref.map.counts >= min_points).sum())
        assert 0 < got['qualified'] < got['voxels']
        if degenerate is not None:
            assert got['degenerate'] == want['degenerate']
            assert abs(got['entropy'] - want['entropy']) <= 1e-12 * abs(want['entropy'])
        assert abs(got['plane_thickness'] - want['plane_thickness']) <= 1e-12 * want['plane_thickness']
    assert m.sharpness() == m.sharpness(4)
    none = ops.VoxelMap(1.0, capacity=64, moments=True).sharpness()
    assert (none['voxels'], none['qualified'], none['degenerate']) == (0, 0, 0) and np.isnan(none['plane_thickness']) and np.isnan(none['entropy'])


def test_arguments_are_rejected_by_name(ops):
    plain = ops.VoxelMap(0.3, capacity=64)
    with pytest.raises(ValueError, match='moments=True'):
        plain.extract_moments()
    with pytest.raises(ValueError, match='moments=True'):
        plain.sharpness()
    with pytest.raises(ValueError, match='min_points'):
        ops.VoxelMap(0.3, capacity=64, moments=True).sharpness(min_points=0)


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_trajectory_map_sharpness_end_to_end(ops, scans, tmp_path):
    """Three frames of one tiny scan seen from known poses: with --map-sharpness every map line is followed by the report of
    build_map(moments=True) on the same inputs, and the map line and the written map are those of a run without the flag."""
    from rdmnet_amd import trajectory
    rng = np.random.default_rng(9)
    world = with_attribute(scans['s000000'][:3000], 3)
    X = [np.eye(4), random_pose(rng, 3.0), random_pose(rng, 6.0)]
    data, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    frames = [0, 4, 9]
    for f, Xk in zip(frames, X):
        inv = np.linalg.inv(Xk)
        local = world.copy()
        local[:, :3] = (world[:, :3].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        np.save(folder / ('%06d.npy' % f), local)
    for k in range(2):
        T = np.linalg.inv(X[k + 1]) @ X[k]
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=T, transform=T, information=np.eye(6))

    def run(name, extra):
        out, lines = tmp_path / name, []
        trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                            '--map-voxel', '1.0', *extra]), emit=lines.append)
        return lines, open(out / '5_chained_map.npy', 'rb').read()

    plain, plain_bytes = run('plain', [])
    lines, with_bytes = run('sharp', ['--map-sharpness'])
    assert not any(' sharpness: ' in s for s in plain)
    assert [s for s in lines if ' sharpness: ' not in s] == plain and with_bytes == plain_bytes
    at = [i for i, s in enumerate(lines) if ' map: ' in s]
    assert len(at) == 1 and lines[at[0] + 1].startswith('seq 5 chained sharpness: ')
    assert re.fullmatch(r'seq 5 chained sharpness: \d+ of \d+ voxels with >= 4 points, plane thickness \d+\.\d{3} mm, entropy -?\d+\.\d{4} '
                        r'\(\d+ degenerate\)', lines[at[0] + 1]), lines[at[0] + 1]
    nodes = trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0]
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    vmap = trajectory.build_map(paths, nodes, voxel=1.0, moments=True)
    assert lines[at[0] + 1] == trajectory.sharpness_line(5, 'chained', 4, vmap.sharpness(4))
    want = MR.build([np.load(p) for p in paths], nodes, 1.0).sharpness(4)
    got = vmap.sharpness(4)
    assert (got['voxels'], got['qualified']) == (want['voxels'], want['qualified']) and got['qualified'] > 0
    assert abs(got['plane_thickness'] - want['plane_thickness']) <= 1e-12 * want['plane_thickness']
    six, _ = run('six', ['--map-sharpness', '--map-sharpness-min-points', '6', '--optimize'])
    assert sum(' sharpness: ' in s and '>= 6 points' in s for s in six) == 2 and any(s.startswith('seq 5 optimized sharpness: ') for s in six)
