"""GPU: the robust weights of the scan-to-map registration (rdm_voxel_map_register_robust, ops.VoxelMap.register(robust_scale=...),
`trajectory --map-refine --map-refine-robust`) against the NumPy restatement tests/voxel_register_robust_restatement.py: the
weighted evaluation alone within the summation bound, five forced updates, bit equality of the weighted form across runs, batch
positions, capacities and integration orders, off means the plain form bit for bit, recovery where a box stands elsewhere in the scan
than in the map, the argument errors by name, and one command-line run.

The scene is test_voxel_register's street, 4 000 points a scan, with a box of 400 points that stands 0.3 m further in x and y in the
registered scan (index 4) than in the seven scans of the maps (0.3 m and 1 m voxels); robust_scale 9."""
import os

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_register_robust_restatement as WR
from test_voxel_register import perturb, pose_error

pytestmark = pytest.mark.gpu

VOXELS = (0.3, 1.0)
SIGMA = 0.02
SCALE = 9.0
ERR_ARG = -1  # RDM_ERR_ARG
# The largest entry-wise difference between the library's pose and the restatement's after five weighted updates, measured over the
# four cases of test_five_weighted_updates_agree_with_the_restatement: 2.8e-16 (rotation entries and metres alike; 2.8e-17, 2.2e-16,
# 1.1e-16 and 2.8e-16 in the cases' order).  The asserted bound is 100 times that (test_voxel_register_gpu's rule: the margin is for a
# point within rounding of a cell face that takes the other voxel in one of the two computations), far below the cap of 1e-9.
POSE_MEASURED = 2.8e-16
POSE_BOUND = 100.0 * POSE_MEASURED
_cache = {}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def scene():
    """Computed once, never changed: the clouds, the true poses, the seven map scans and per voxel size the restatement's map of them."""
    if 'scene' not in _cache:
        clouds, poses = WR.moved_box(np.random.default_rng(6), 400)
        others = [k for k in range(len(clouds)) if k != 4]
        tables = {v: MR.build([clouds[k] for k in others], poses[others], v, 3) for v in VOXELS}
        _cache['scene'] = (clouds, poses, others, tables)
    return _cache['scene']


def cuda(cloud):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).cuda()


def gpu_map(ops, voxel, order=None, capacity=1 << 16):
    clouds, poses, others, _ = scene()
    order = others if order is None else order
    return ops.VoxelMap(voxel, channels=3, capacity=capacity, moments=True).integrate([cuda(clouds[k]) for k in order], poses[order])


def shared_map(ops, voxel):
    if ('map', voxel) not in _cache:
        _cache['map', voxel] = gpu_map(ops, voxel)
    return _cache['map', voxel]


def starts(seeds=(3, 4), sigma_t=0.05, sigma_r=0.005):
    _, poses, _, _ = scene()
    return np.stack([perturb(poses[4], np.random.default_rng(s), sigma_t, sigma_r) for s in seeds])


def outputs(res):
    out = (res.transformations, res.information, res.gradient, res.cost, res.iterations, res.num_correspondences, res.num_points, res.status)
    return out if res.weight_sum is None else out + (res.weight_sum,)


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    import torch
    A, B = outputs(a), outputs(b)
    return len(A) == len(B) and all(torch.equal(x[rows_a], y[rows_b]) for x, y in zip(A, B))


# ---- the evaluation alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
def test_weighted_evaluation_is_within_the_summation_bound(ops, voxel, neighbors):
    """max_iteration = 0, robust_scale 9.  Counts exactly; every entry of H, g, cost and weight_sum within
        2^-52 (n_corr + 192 kappa + 12) A
    of the restatement's, A = the restatement's sum of the absolute values of that entry's weighted terms, kappa = (voxel^2 +
    sigma^2) / sigma^2.  The plain test's bound is 2^-52 (n_corr + 64 kappa) A: n_corr u for a sum of n_corr terms in another order
    (u = 2^-52), and e = 64 kappa u for the relative difference of one term x, the differently ordered 3 x 3 inverse in it.  A
    weighted term is l x with l = s s, s = mu / (mu + d2), and d2 is itself a plain term (the cost's), so the two sides' d2 differ
    by e relatively.  d s / s = -(d2 / (mu + d2)) d(d2) / d2, at most e in size; the addition and the division round once each on
    each side, so the two s differ by e + 4 u; the two l by twice that and one rounding each, 2 e + 10 u; the two l x by e more and
    one rounding each: 3 e + 12 u = (192 kappa + 12) u.  The cost's term s d2 (2 e + 6 u) and weight_sum's term l (2 e + 10 u) lie
    within the same constant.  Measured: the largest ratio to the bound over the four cases is 4.6e-4 (2.1e-4, 4.6e-4, 4.9e-5
    and 1.2e-4 in the cases' order)."""
    clouds, poses, _, tables = scene()
    X = np.concatenate([starts(), poses[4:5]])
    res = shared_map(ops, voxel).register([cuda(clouds[4])] * 3, X, sigma=SIGMA, neighbors=neighbors, max_iteration=0, robust_scale=SCALE)
    assert res.status.tolist() == [0, 0, 0] and res.iterations.tolist() == [0, 0, 0]
    assert np.array_equal(res.transformations.cpu().numpy(), X)
    H, g, cost, wsum = (t.cpu().numpy() for t in (res.information, res.gradient, res.cost, res.weight_sum))
    assert wsum.dtype == np.float64 and wsum.shape == (3,)
    kappa = (voxel ** 2 + SIGMA ** 2) / SIGMA ** 2
    worst = 0.0
    for s in range(3):
        e = WR.evaluate(tables[voxel], clouds[4], X[s], SIGMA, 4, neighbors, robust_scale=SCALE)
        assert int(res.num_correspondences[s]) == e['n_corr'] and int(res.num_points[s]) == e['n_points'] == len(clouds[4])
        assert e['n_corr'] > 300 and 0.0 < wsum[s] < e['n_corr']
        bound = 2.0 ** -52 * (e['n_corr'] + 192.0 * kappa + 12.0)
        ratios = [np.abs(H[s] - e['H']) / (bound * e['abs_H']), np.abs(g[s] - e['g']) / (bound * e['abs_g']),
                  np.abs(cost[s] - e['cost']) / (bound * e['abs_cost']), np.abs(wsum[s] - e['weight_sum']) / (bound * e['abs_weight_sum'])]
        worst = max([worst] + [float(np.max(r)) for r in ratios])
        assert all(np.max(r) <= 1.0 for r in ratios), (s, [float(np.max(r)) for r in ratios])
        assert np.array_equal(H[s], H[s].T)
    print(f'voxel {voxel}, neighbors {neighbors}: largest |difference| / bound = {worst:.3e}')


# ---- a fixed number of updates ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('voxel', VOXELS)
def test_five_weighted_updates_agree_with_the_restatement(ops, voxel, neighbors):
    clouds, _, _, tables = scene()
    X = starts((3,))
    res = shared_map(ops, voxel).register([cuda(clouds[4])], X, sigma=SIGMA, neighbors=neighbors, max_iteration=5, rot_eps=0.0, trans_eps=0.0,
                                          robust_scale=SCALE)
    assert res.status.tolist() == [0] and res.iterations.tolist() == [5]
    T = res.transformations.cpu().numpy()
    want = WR.register(tables[voxel], clouds[4], X[0], SIGMA, 4, neighbors, 5, 0.0, 0.0, robust_scale=SCALE)
    assert want['status'] == 0 and want['iterations'] == 5
    diff = float(np.abs(T[0] - want['transform']).max())
    print(f'voxel {voxel}, neighbors {neighbors}: largest pose difference {diff:.3e}')
    assert diff <= POSE_BOUND <= 1e-9
    assert int(res.num_correspondences[0]) == want['n_corr']
    assert abs(float(res.weight_sum[0]) - want['weight_sum']) <= 1e-9 * want['weight_sum']
    assert T[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]


# ---- bit equality of the weighted form ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
def test_runs_batch_positions_and_an_empty_scan_do_not_change_a_bit(ops, neighbors):
    import torch
    clouds, poses, _, _ = scene()
    vmap = shared_map(ops, 0.3)
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=neighbors, max_iteration=6, robust_scale=SCALE)
    alone = vmap.register([cuda(clouds[4])], X[:1], **kw)
    assert same(alone, vmap.register([cuda(clouds[4])], X[:1], **kw))
    assert int(alone.iterations[0]) >= 1 and int(alone.num_correspondences[0]) > 300
    assert 0.0 < float(alone.weight_sum[0]) < int(alone.num_correspondences[0])
    empty = torch.zeros((0, 3), dtype=torch.float32, device='cuda')
    batch = [cuda(clouds[2]), empty, cuda(clouds[4]), cuda(clouds[6][:1000]), cuda(clouds[4]), empty]
    Xb = np.stack([poses[2], np.eye(4), X[0], poses[6], X[0], X[1]])
    both = vmap.register(batch, Xb, **kw)
    assert same(both, vmap.register(batch, Xb, **kw))
    assert same(alone, both, rows_b=slice(2, 3)) and same(alone, both, rows_b=slice(4, 5))
    first = vmap.register([cuda(clouds[4]), cuda(clouds[1])], np.stack([X[0], poses[1]]), **kw)
    assert same(alone, first, rows_b=slice(0, 1))
    # an empty scan is degenerate where it stands, moves nothing and weighs nothing
    assert both.status[[1, 5]].tolist() == [2, 2] and both.num_points[[1, 5]].tolist() == [0, 0]
    assert both.weight_sum[[1, 5]].tolist() == [0.0, 0.0]
    assert np.array_equal(both.transformations[[1, 5]].cpu().numpy(), Xb[[1, 5]])


def near(cloud, n):
    return cloud[np.argsort(np.linalg.norm(cloud, axis=1), kind='stable')[:n]]


def test_capacity_and_growth_do_not_change_a_bit(ops):
    clouds, poses, _, _ = scene()
    part = near(clouds[3], 1500)
    query, X = cuda(near(clouds[4], 1500)), starts()
    small = ops.VoxelMap(1.0, channels=3, capacity=1 << 12, moments=True).integrate([cuda(part)], poses[3:4])
    assert small.capacity == 1 << 12
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4, robust_scale=SCALE)
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
    kw = dict(sigma=SIGMA, neighbors=7, max_iteration=4, robust_scale=SCALE)
    a = shared_map(ops, 1.0).register([cuda(clouds[4])] * 2, X, **kw)
    b = gpu_map(ops, 1.0, order=others[::-1], capacity=1 << 17).register([cuda(clouds[4])] * 2, X, **kw)
    assert same(a, b)


# ---- off means plain -------------------------------------------------------------------------------------------------------------

def raw_call(vmap, pts, off, X, n_scans, robust_scale, weight_sums, neighbors=1, max_iteration=4):
    """rdm_voxel_map_register_robust on fresh zeroed outputs -> (code, real [n, 59], stats [n, 4])."""
    import torch
    from rdmnet_amd import _lib
    L = _lib.lib()
    n = max(n_scans, 1)
    out = torch.zeros((59 * n,), dtype=torch.float64, device='cuda')
    stats = torch.zeros((n, 4), dtype=torch.int64, device='cuda')
    ws = torch.empty((L.rdm_voxel_map_register_workspace_bytes(n),), dtype=torch.uint8, device='cuda')
    code = L.rdm_voxel_map_register_robust(*vmap._head(), vmap._mom.data_ptr(), vmap._mom.numel(), vmap.voxel, pts.data_ptr(), 3, len(pts),
                                           off.data_ptr(), X.data_ptr(), n_scans, 0.0, float('inf'), SIGMA, 4, neighbors, max_iteration, 1e-5,
                                           1e-4, robust_scale, out[0:].data_ptr(), out[16 * n:].data_ptr(), out[52 * n:].data_ptr(),
                                           out[58 * n:].data_ptr(), 0 if weight_sums is None else weight_sums.data_ptr(), stats.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return code, out, stats


@pytest.mark.parametrize('neighbors', (1, 7))
def test_off_is_the_plain_form_bit_for_bit(ops, neighbors):
    import torch
    clouds, _, _, _ = scene()
    vmap = shared_map(ops, 1.0)
    X = starts()
    kw = dict(sigma=SIGMA, neighbors=neighbors, max_iteration=4)
    plain = vmap.register([cuda(clouds[4])] * 2, X, **kw)
    none = vmap.register([cuda(clouds[4])] * 2, X, robust_scale=None, **kw)
    assert plain.weight_sum is None and none.weight_sum is None and same(plain, none)
    assert 'by weight' not in repr(plain)
    pts = torch.cat([cuda(clouds[4])] * 2)
    off = torch.tensor([0, len(clouds[4]), 2 * len(clouds[4])], dtype=torch.int64, device='cuda')
    Xd = torch.from_numpy(X.copy()).cuda()
    code, out, stats = raw_call(vmap, pts, off, Xd, 2, 0.0, None, neighbors)
    assert code == 0
    assert torch.equal(out[:32].view(2, 4, 4), plain.transformations) and torch.equal(out[32:104].view(2, 6, 6), plain.information)
    assert torch.equal(out[104:116].view(2, 6), plain.gradient) and torch.equal(out[116:118], plain.cost)
    assert torch.equal(stats, torch.stack([plain.iterations, plain.num_correspondences, plain.num_points, plain.status], 1))
    # with a buffer, scale 0 says that every pair has weight one
    wsum = torch.full((2,), -1.0, dtype=torch.float64, device='cuda')
    code, out2, stats2 = raw_call(vmap, pts, off, Xd, 2, 0.0, wsum, neighbors)
    assert code == 0 and torch.equal(out2, out) and torch.equal(stats2, stats)
    assert torch.equal(wsum, plain.num_correspondences.double()) and int(plain.num_correspondences.min()) > 300
    # and the weights do change the result
    weighted = vmap.register([cuda(clouds[4])] * 2, X, robust_scale=SCALE, **kw)
    assert not torch.equal(weighted.transformations, plain.transformations) and 'by weight' in repr(weighted)
    # the positional constructor of before
    r = ops.MapRegistrationResult(*outputs(plain))
    assert r.weight_sum is None and repr(r) == repr(plain)


# ---- recovery --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
def test_recovery_where_the_box_stands_elsewhere(ops, neighbors):
    """The restatement's weighted pose errors are below a third of its plain ones (checked first), and so are the library's of the
    library's."""
    clouds, poses, _, tables = scene()
    vmap = shared_map(ops, 1.0)
    X0 = starts((3,))
    ref_plain = WR.register(tables[1.0], clouds[4], X0[0], neighbors=neighbors)
    ref_weighted = WR.register(tables[1.0], clouds[4], X0[0], neighbors=neighbors, robust_scale=SCALE)
    a, b = pose_error(ref_plain['transform'], poses[4]), pose_error(ref_weighted['transform'], poses[4])
    assert b[0] < a[0] / 3.0 and b[1] < a[1] / 3.0
    plain = vmap.register([cuda(clouds[4])], X0, neighbors=neighbors)
    weighted = vmap.register([cuda(clouds[4])], X0, neighbors=neighbors, robust_scale=SCALE)
    c = pose_error(plain.transformations[0].cpu().numpy(), poses[4])
    d = pose_error(weighted.transformations[0].cpu().numpy(), poses[4])
    print(f'neighbors {neighbors}: plain {c[0] * 100:.2f} cm / {c[1] * 1e3:.2f} mrad, weighted {d[0] * 100:.2f} cm / {d[1] * 1e3:.2f} mrad '
          f'(restatement {a[0] * 100:.2f} / {a[1] * 1e3:.2f} and {b[0] * 100:.2f} / {b[1] * 1e3:.2f}); {weighted!r}')
    assert plain.status.tolist() == [1] and weighted.status.tolist() == [1]
    assert d[0] < c[0] / 3.0 and d[1] < c[1] / 3.0


# ---- argument errors -------------------------------------------------------------------------------------------------------------

def test_arguments_are_rejected_by_name(ops):
    import torch
    from rdmnet_amd import _lib
    clouds, poses, _, _ = scene()
    vmap = shared_map(ops, 1.0)
    pts = cuda(clouds[4][:500])
    for bad in (0, -1, float('nan'), float('inf'), '9', 0.0, -0.5):
        with pytest.raises(ValueError, match='robust_scale'):
            vmap.register([pts], poses[4:5], robust_scale=bad)
    off = torch.tensor([0, 500], dtype=torch.int64, device='cuda')
    X = torch.from_numpy(poses[4:5].copy()).cuda()
    for bad in (-1.0, -1e-300, float('nan'), float('inf'), float('-inf')):
        wsum = torch.zeros((1,), dtype=torch.float64, device='cuda')
        code, out, stats = raw_call(vmap, pts, off, X, 1, bad, wsum)
        assert code == ERR_ARG and b'robust_scale' in _lib.lib().rdm_last_error(), bad
        assert not out.any() and not stats.any() and not wsum.any()  # nothing ran
    # the plain form's errors come first and keep its name
    code, _, _ = raw_call(vmap, pts, off, X, 1, SCALE, None, neighbors=3)
    assert code == ERR_ARG and b'rdm_voxel_map_register: neighbors must be 1 or 7' in _lib.lib().rdm_last_error()
    # a null weight_sums is valid with weights on, and an empty batch writes nothing
    code, out, stats = raw_call(vmap, pts, off, X, 1, SCALE, None, max_iteration=0)
    want = vmap.register([pts], poses[4:5], max_iteration=0, robust_scale=SCALE)
    assert code == 0 and torch.equal(out[16:52].view(6, 6), want.information[0]) and torch.equal(out[58:59], want.cost)
    wsum = torch.zeros((1,), dtype=torch.float64, device='cuda')
    code, out, stats = raw_call(vmap, pts, off, X, 0, SCALE, wsum)
    assert code == 0 and not out.any() and not stats.any() and not wsum.any()
    res = vmap.register([], np.zeros((0, 4, 4)), robust_scale=SCALE)
    assert res.weight_sum.shape == (0,) and res.weight_sum.dtype == torch.float64 and repr(res) == 'MapRegistrationResult()'


# ---- the command line ------------------------------------------------------------------------------------------------------------

def test_trajectory_map_refine_robust_end_to_end(ops, tmp_path):
    """Four frames of the scene with pair poses off by 5 cm / 5 mrad: --map-refine-robust 9 changes the `refined` lines and files of a
    --map-refine run, adds the one `robust weights` line directly after the `refined against the map` line, and leaves every other
    line and file byte for byte."""
    from rdmnet_amd import trajectory
    clouds, poses, _, _ = scene()
    frames = [0, 3, 6, 9]
    at = [2, 3, 4, 5]  # the scans around the one in which the box stands elsewhere
    data, pairs = tmp_path / 'data', tmp_path / 'pairs'
    folder = data / 'downsampled_xyzi' / '05'
    os.makedirs(folder)
    pairs.mkdir()
    rng = np.random.default_rng(31)
    noisy = [poses[at[0]]] + [perturb(poses[k], rng, 0.05, 0.005) for k in at[1:]]
    for k, f in enumerate(frames):
        np.save(folder / ('%06d.npy' % f), clouds[at[k]])
    for k in range(3):
        np.savez(pairs / f'5_{frames[k]}_{frames[k + 1]}.npz', estimated_transform=np.linalg.inv(noisy[k + 1]) @ noisy[k],
                 transform=np.linalg.inv(poses[at[k + 1]]) @ poses[at[k]], information=np.eye(6))

    def run(name, extra):
        out, lines = tmp_path / name, []
        trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(out),
                                                            '--map-voxel', '1.0', '--map-sharpness', '--map-refine', '--map-refine-neighbors',
                                                            '7', '--map-refine-iterations', '20', *extra]), emit=lines.append)
        return lines, out

    plain, plain_out = run('plain', [])
    lines, out = run('robust', ['--map-refine-robust', '9'])
    assert not any('robust weights' in s for s in plain)
    added = [k for k, s in enumerate(lines) if 'robust weights' in s]
    assert len(added) == 1 and lines[added[0] - 1].startswith('seq 5 refined against the map: ')
    rest = lines[:added[0]] + lines[added[0] + 1:]
    assert len(rest) == len(plain)
    refined = [k for k, s in enumerate(plain) if ' refined' in s]
    assert len(refined) == 4 and all((' refined' in rest[k]) == (k in refined) for k in range(len(rest)))
    assert all(rest[k] == plain[k] for k in range(len(rest)) if k not in refined)
    assert [rest[k] for k in refined] != [plain[k] for k in refined] and rest[refined[0]] != plain[refined[0]]  # the error line differs
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain_out)) == ['5_chained.txt', '5_chained_map.npy', '5_refined.txt', '5_refined_map.npy']
    for name in os.listdir(plain_out):
        assert (open(out / name, 'rb').read() == open(plain_out / name, 'rb').read()) == ('refined' not in name), name
    paths = [str(folder / ('%06d.npy' % f)) for f in frames]
    base = trajectory.sequence_graph(trajectory.read_sequences(str(pairs))[5])[0]
    again, _, stats = trajectory.refine_against_map(paths, base, voxel=1.0, neighbors=7, max_iteration=20, robust_scale=9)
    assert stats['weights'].shape == (4,) and stats['weights'][0] == 0.0
    assert (stats['weights'][1:] > 0).all() and (stats['weights'][1:] < stats['correspondences'][1:]).all()
    assert lines[added[0]] == trajectory.robust_line(5, 'refined', 9.0, stats) and lines[added[0] - 1] == trajectory.refine_line(5, stats)
    assert lines[added[0]].startswith('seq 5 refined robust weights: scale 9, ') and lines[added[0]].endswith(' correspondences per frame by weight')
    text = open(out / '5_refined.txt').read().splitlines()
    written = np.array([[float(v) for v in row.split()] + [0, 0, 0, 1] for row in text]).reshape(4, 4, 4)
    assert np.abs(again - written).max() < 1e-8  # (the file holds nine decimals)
    assert 'weights' not in trajectory.refine_against_map(paths, base, voxel=1.0, neighbors=7, max_iteration=20)[2]


def test_localize_against_map_passes_the_scale_on(ops, tmp_path):
    from rdmnet_amd import trajectory
    clouds, poses, _, _ = scene()
    vmap = shared_map(ops, 1.0)
    paths = []
    for k in (4, 4):
        paths.append(str(tmp_path / f'{len(paths)}.npy'))
        np.save(paths[-1], clouds[k])
    X = starts()
    want = vmap.register([cuda(clouds[4])] * 2, X, robust_scale=SCALE)
    got, stats = trajectory.localize_against_map(paths, X, vmap, robust_scale=SCALE)
    assert np.array_equal(got, want.transformations.cpu().numpy()) and np.array_equal(stats['weights'], want.weight_sum.cpu().numpy())
    assert trajectory.robust_line(5, 'localized', SCALE, stats).startswith('seq 5 localized robust weights: scale 9, ')
    assert 'weights' not in trajectory.localize_against_map(paths, X, vmap)[1]
