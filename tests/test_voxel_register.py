"""CPU: the scan-to-map registration's declarations and bindings, the `--map-refine` options of `python -m rdmnet_amd.trajectory` that
need no GPU, and the NumPy restatement tests/voxel_register_restatement.py itself: its Jacobian and update convention against
finite differences of its own cost, recovery of a perturbed pose, and what the registration is for -- sequential refinement of a
noisy trajectory makes the map sharper and the poses better.

The scene (`street`) is closed in x, unlike test_voxel_moments.ground_and_walls: a ground plane, two side walls and two cross walls,
so all six degrees of freedom of a pose are constrained."""
import os
import re

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_register_restatement as RR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
NEW = ('rdm_voxel_map_register_workspace_bytes', 'rdm_voxel_map_register')


def street(rng, n_scans=8, per_scan=6000, range_noise=0.02, max_range=30.0):
    """Ground (z = 0, x from -2 to 40 m, y within +-8 m), side walls at y = +-8 m and cross walls at x = -2 and 40 m, all 4 m high,
    seen from n_scans poses 3 m apart along x, 1.7 m above the ground: every scan samples the surfaces (half of its points on the
    ground, a sixth on each side wall, a twelfth on each cross wall), moves each sample along its ray by N(0, range_noise), keeps
    what lies within max_range and stores it in the sensor frame.  The map straddles the world origin: cells are negative in x and y.
    -> (clouds float32 [<= per_scan, 3], true poses [n, 4, 4])."""
    clouds, poses = [], []
    for k in range(n_scans):
        yaw = 0.05 * np.sin(k)
        X = np.eye(4)
        X[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        X[:3, 3] = [2.0 + 3.0 * k, 0.3 * np.cos(k), 1.7]
        n_g, n_s = per_scan // 2, per_scan // 6
        n_c = (per_scan - n_g - 2 * n_s) // 2
        ground = np.stack([rng.uniform(-2, 40, n_g), rng.uniform(-8, 8, n_g), np.zeros(n_g)], 1)
        side = [np.stack([rng.uniform(-2, 40, n_s), np.full(n_s, y), rng.uniform(0, 4, n_s)], 1) for y in (-8.0, 8.0)]
        cross = [np.stack([np.full(n_c, x), rng.uniform(-8, 8, n_c), rng.uniform(0, 4, n_c)], 1) for x in (-2.0, 40.0)]
        world = np.concatenate([ground] + side + cross)
        ray = world - X[:3, 3]
        dist = np.linalg.norm(ray, axis=1, keepdims=True)
        world = X[:3, 3] + ray * (1.0 + rng.normal(0.0, range_noise, dist.shape) / dist)
        world = world[dist[:, 0] < max_range]
        inv = np.linalg.inv(X)
        clouds.append((world @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        poses.append(X)
    return clouds, np.stack(poses)


def perturb(X, rng, sigma_t, sigma_r):
    """X moved by Exp(omega), + v with omega ~ N(0, sigma_r) and v ~ N(0, sigma_t) per axis."""
    return RR.apply(X, np.concatenate([rng.normal(0.0, sigma_r, 3), rng.normal(0.0, sigma_t, 3)]))


def pose_error(X, truth):
    """(translation error in metres, rotation angle in radians)."""
    E = X[:3, :3] @ truth[:3, :3].T
    return float(np.linalg.norm(X[:3, 3] - truth[:3, 3])), float(np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0)))


def refine_sequentially(clouds, base, voxel, **kw):
    """trajectory.refine_against_map restated on the restatements -> (refined poses, the Moments map, degenerate frames)."""
    table = MR.Moments(voxel, 3).integrate([clouds[0]], [base[0]])
    out, degenerate = [base[0]], 0
    for k in range(1, len(clouds)):
        init = out[k - 1] @ np.linalg.inv(base[k - 1]) @ base[k]
        res = RR.register(table, clouds[k], init, **kw)
        degenerate += res['status'] == 2
        out.append(init if res['status'] == 2 else res['transform'])
        table.integrate([clouds[k]], [out[k]])
    return np.stack(out), table, degenerate


def test_header_declares_the_entry_points_and_bindings_have_them():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r'^(?:size_t|int) ' + name + r'\(([^;]*)\);', text, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()]), name
    assert 'tests/voxel_register_restatement.py' in text
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)  # new entry points do not bump it
    # the map's head, the moments block, the voxel and integrate's batch come first, as in rdm_voxel_map_integrate_moments
    sig = _lib.SIGNATURES['rdm_voxel_map_register'][1]
    assert sig[:4] == _lib.SIGNATURES['rdm_voxel_map_integrate'][1][:4] and sig[4:6] == [_lib.c_void, _lib.c_size]
    assert sig[6:15] == _lib.SIGNATURES['rdm_voxel_map_integrate'][1][4:13]


def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_refine_options_parse_and_need_map_scans_and_out(tmp_path):
    a = parse(['--features-root', 'x'])
    assert a.map_refine is False and (a.map_refine_sigma, a.map_refine_neighbors, a.map_refine_iterations) == (0.02, 1, 30)
    a = parse(['--features-root', 'x', '--map-scans', 'R', '--out', 'o', '--map-refine', '--map-refine-sigma', '0.05', '--map-refine-neighbors',
               '7', '--map-refine-iterations', '12'])
    assert a.map_refine is True and (a.map_refine_sigma, a.map_refine_neighbors, a.map_refine_iterations) == (0.05, 7, 12)
    with pytest.raises(SystemExit):
        parse(['--features-root', 'x', '--map-refine-neighbors', '3'])
    pairs = tmp_path / 'pairs'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    lines = []
    base = ['--features-root', str(pairs)]
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine needs --map-scans and --out'):
        trajectory.run(parse(base + ['--map-refine']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine needs --map-scans and --out'):
        trajectory.run(parse(base + ['--map-refine', '--map-scans', str(tmp_path)]), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine needs --map-scans and --out'):
        trajectory.run(parse(base + ['--map-refine', '--out', str(tmp_path / 'o')]), emit=lines.append)
    for flag, value in (('--map-refine-sigma', '0.1'), ('--map-refine-neighbors', '7'), ('--map-refine-iterations', '3')):
        with pytest.raises(trajectory.TrajectoryError, match=flag + ' needs --map-refine'):
            trajectory.run(parse(base + [flag, value]), emit=lines.append)
    for flag, value in (('--map-refine-sigma', '0'), ('--map-refine-iterations', '-1')):
        with pytest.raises(trajectory.TrajectoryError, match='--map-refine-sigma must be > 0 and --map-refine-iterations >= 0'):
            trajectory.run(parse(base + ['--map-refine', '--map-scans', str(tmp_path), '--out', str(tmp_path / 'o'), flag, value]),
                           emit=lines.append)
    assert lines == []  # found before anything is reported
    with pytest.raises(SystemExit, match='--map-refine needs --map-scans and --out'):
        trajectory.main(base + ['--map-refine'])


def test_refine_line_format():
    stats = dict(frames=5, iterations=np.array([0, 4, 6, 5, 5]), correspondences=np.array([0, 100, 200, 300, 400]), degenerate=1)
    assert trajectory.refine_line(3, stats) == ('seq 3 refined against the map: 5 frames, 5.00 iterations and 250 correspondences per frame, '
                                                '1 degenerate frames')


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_exp_and_apply_conventions():
    R = RR.exp_so3([0.0, 0.0, np.pi / 2])
    assert np.abs(R - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-15
    assert np.abs(RR.exp_so3([1e-6, -2e-6, 3e-6]) - (np.eye(3) + RR.skew([1e-6, -2e-6, 3e-6])[0])).max() < 1e-11
    X = np.eye(4)
    X[:3, 3] = [10.0, 0.0, 0.0]
    Y = RR.apply(X, np.array([0.0, 0.0, np.pi / 2, 1.0, 2.0, 3.0]))
    assert np.abs(Y[:3, :3] - R).max() < 1e-15 and Y[:3, 3].tolist() == [11.0, 2.0, 3.0]  # the rotation turns about the sensor, not the origin
    assert RR.cholesky_solve(np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), np.ones(6)) is None
    assert RR.cholesky_solve(np.diag([1.0, 1.0, np.nan, 1.0, 1.0, 1.0]), np.ones(6)) is None
    A = np.random.default_rng(0).normal(size=(6, 6))
    H, g = A @ A.T + np.eye(6), np.arange(6.0)
    assert np.abs(H @ RR.cholesky_solve(H, g) + g).max() < 1e-12


def test_cost_is_quadratic_in_the_update_with_the_stated_gradient_and_hessian():
    """Points well inside their voxels (the middle half of each edge), voxels of eight points each, a pose far from the origin: for
    a small delta no association changes, so the cost is a smooth function of delta.  H is the Gauss-Newton matrix: it leaves out
    the curvature of the residual, r(delta) = r + J delta + omega x (omega x q) / 2 + ..., so the cost's own second order is
    delta^T H delta + c with c = sum (M r).(omega x (omega x q)), which is not small where r is not (the six neighbours' residuals
    are a voxel long).  The test computes c from the restatement's per-pair terms and checks
        cost(Exp(delta) X) - cost(X) = 2 g.delta + delta^T H delta + c + O(|delta|^3);
    for a pure translation c = 0 and the difference is the quadratic exactly.  A wrong Jacobian, a wrong sign or a perturbation
    about the origin instead of the sensor breaks the first or the second order.  The cubic terms are (J delta)^T M (omega x (omega x
    q)) and (M r).(omega x (omega x (omega x q))) / 3, at most sum |M| (|q|^2 + |r| |q| / 3) |delta|^3 <= 4 sum |M| |q|^2 |delta|^3 here
    (|r| < 2 m, |q| > 1 m for almost every point), and sum |M| |q|^2 <= 3 trace(H's rotation block)."""
    rng = np.random.default_rng(4)
    voxel = 1.0
    cells = np.array([(a, b, c) for a in range(-3, 3) for b in range(-2, 2) for c in range(-1, 2)])
    world = np.concatenate([(cells + rng.uniform(0.3, 0.7, (len(cells), 3))) * voxel for _ in range(8)]) + np.array([500.0, -300.0, 20.0])
    table = MR.build([world.astype(np.float32)], [np.eye(4)], voxel, 3)
    X = perturb(np.eye(4), rng, 0.3, 0.5)
    X[:3, 3] += [500.0, -300.0, 20.0]
    inv = np.linalg.inv(X)
    scan = (world[::2] + rng.normal(0, 0.03, world[::2].shape)) @ inv[:3, :3].T + inv[:3, 3]
    scan = scan.astype(np.float32)
    for neighbors in (1, 7):
        e = RR.evaluate(table, scan, X, sigma=0.05, min_points=4, neighbors=neighbors, terms=True)
        assert e['n_points'] == len(scan) and e['n_corr'] >= len(scan)
        assert np.abs(e['H'] - e['H'].T).max() <= 1e-9 * np.abs(e['H']).max()
        Mr = (e['M'] @ e['r'][:, :, None])[:, :, 0]
        cubic = 12.0 * np.trace(e['H'][:3, :3])
        for scale in (1e-3, 1e-4):
            for kind in ('both', 'both', 'rotation', 'translation'):
                delta = rng.normal(0, 1, 6)
                if kind != 'both':
                    delta[3 if kind == 'rotation' else 0:][:3] = 0.0
                delta *= scale / np.linalg.norm(delta)
                moved = RR.evaluate(table, scan, RR.apply(X, delta), sigma=0.05, min_points=4, neighbors=neighbors)
                assert moved['n_corr'] == e['n_corr']
                first, second = 2.0 * e['g'] @ delta, delta @ e['H'] @ delta
                curvature = float((Mr * np.cross(delta[:3], np.cross(delta[:3], e['q']))).sum())
                got = moved['cost'] - e['cost']
                rounding = 1e-12 * e['abs_cost']
                bound = (cubic * scale ** 3 if kind != 'translation' else 0.0) + rounding
                print(f'neighbors {neighbors}, |delta| {scale:g} ({kind}): {got:.6e} = {first:.6e} + {second:.6e} + {curvature:.6e} + '
                      f'{got - (first + second + curvature):.2e} (bound {bound:.2e})')
                assert abs(got - (first + second + curvature)) <= bound, (neighbors, scale, kind)
                assert scale > 1e-4 or abs(second) > 10 * bound  # at the smaller step the check can tell the second order
                assert kind != 'translation' or curvature == 0.0


def test_recovery_from_5_cm_and_5_mrad():
    rng = np.random.default_rng(5)
    clouds, poses = street(rng, per_scan=6000)
    for voxel in (0.3, 1.0):
        table = MR.build(clouds[:4] + clouds[5:], np.concatenate([poses[:4], poses[5:]]), voxel, 3)
        for seed in (11, 12):
            X0 = perturb(poses[4], np.random.default_rng(seed), 0.05, 0.005)
            res = RR.register(table, clouds[4], X0, neighbors=1)
            before, after = pose_error(X0, poses[4]), pose_error(res['transform'], poses[4])
            print(f'voxel {voxel}: {before[0] * 100:.2f} cm / {before[1] * 1e3:.2f} mrad -> {after[0] * 100:.2f} cm / {after[1] * 1e3:.2f} mrad, '
                  f"{res['iterations']} updates, status {res['status']}, {res['n_corr']} pairs")
            assert res['status'] == 1 and after[0] < 0.5 * before[0] and after[1] < 0.5 * before[1]
            zero = RR.register(table, clouds[4], X0, max_iteration=0)
            assert zero['status'] == 0 and zero['iterations'] == 0 and np.array_equal(zero['transform'], X0)


def test_sequential_refinement_sharpens_the_map_and_improves_the_poses():
    """Frames 1 .. 7 perturbed by 5 cm / 5 mrad per axis, frame 0 (the anchor) exact.  Scans of 16 000 points: the smallest of
    10 000, 14 000, 16 000 and 20 000 at which the restatement kept a factor of at least 2.5 on the plane thickness and 2.7 on the mean
    translation error for each of three seeds (at 14 000 one seed kept 1.1 on the error, at 10 000 none kept 2.5); with this seed it
    keeps 2.5 and 3.8.  The assertions are the strict inequalities."""
    rng = np.random.default_rng(2)
    clouds, poses = street(rng, per_scan=16000)
    prng = np.random.default_rng(102)
    noisy = np.stack([poses[0]] + [perturb(X, prng, 0.05, 0.005) for X in poses[1:]])
    refined, table, degenerate = refine_sequentially(clouds, noisy, 0.3)
    err_noisy = np.mean([pose_error(a, b)[0] for a, b in zip(noisy[1:], poses[1:])])
    err_refined = np.mean([pose_error(a, b)[0] for a, b in zip(refined[1:], poses[1:])])
    thick_noisy = MR.build(clouds, noisy, 0.3, 3).sharpness(4)['plane_thickness']
    thick_refined = table.sharpness(4)['plane_thickness']
    thick_true = MR.build(clouds, poses, 0.3, 3).sharpness(4)['plane_thickness']
    print(f'mean translation error {err_noisy * 100:.2f} -> {err_refined * 100:.2f} cm; plane thickness {thick_noisy * 1e3:.1f} -> '
          f'{thick_refined * 1e3:.1f} mm (true poses: {thick_true * 1e3:.1f} mm); {degenerate} degenerate frames')
    assert degenerate == 0
    assert thick_refined < thick_noisy and err_refined < err_noisy
    assert thick_true < thick_refined  # (no refinement beats the truth)
