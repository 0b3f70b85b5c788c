"""CPU: the voxel moments' declarations and bindings, the `--map-sharpness` options of `python -m rdmnet_amd.trajectory` that need no
GPU, the NumPy restatement tests/voxel_moments_restatement.py on hand-worked voxels, and what the moments are for: the plane
thickness of a map grows with the pose noise while the voxel count does not tell.

The hand-worked voxels use 0.25 m voxels: s = voxel / 4096 = 2^-14 and every coordinate below is a multiple of 2^-22 m of magnitude
below 2 m, exact in float32, so every figure is exact and compared with ==."""
import os
import re

import numpy as np
import pytest

import voxel_map_restatement as VM
import voxel_moments_restatement as MR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
NEW = ('rdm_voxel_moments_bytes', 'rdm_voxel_moments_reset', 'rdm_voxel_map_integrate_moments', 'rdm_voxel_moments_rehash',
       'rdm_voxel_map_extract_moments')
V = 0.25
S = 2.0 ** -14  # V / 4096
EYE = np.eye(4)


def test_header_declares_the_entry_points_and_bindings_have_them():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r'^(?:size_t|int) ' + name + r'\(([^;]*)\);', text, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()]), name
    assert re.search(r'#define RDM_VOXEL_MOMENTS_PLANES 9\b', text) and re.search(r'#define RDM_VOXEL_MOMENTS_SHIFT 8\b', text)
    assert _lib.VOXEL_MOMENTS_PLANES == 9
    assert 'tests/voxel_moments_restatement.py' in text
    assert _lib.ABI_VERSION == 2  # new entry points do not bump it
    # the integrate with moments takes the plain integrate's arguments plus the block (pointer, bytes) before the stream
    plain, with_moments = _lib.SIGNATURES['rdm_voxel_map_integrate'][1], _lib.SIGNATURES['rdm_voxel_map_integrate_moments'][1]
    assert with_moments == plain[:-1] + [_lib.c_void, _lib.c_size] + plain[-1:]


def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_sharpness_options_parse_and_need_map_scans(tmp_path):
    a = parse(['--features-root', 'x'])
    assert a.map_sharpness is False and a.map_sharpness_min_points == 4
    a = parse(['--features-root', 'x', '--map-scans', 'R', '--out', 'o', '--map-sharpness', '--map-sharpness-min-points', '6'])
    assert a.map_sharpness is True and a.map_sharpness_min_points == 6
    pairs = tmp_path / 'pairs'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    lines = []
    with pytest.raises(trajectory.TrajectoryError, match='--map-sharpness needs --map-scans'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-sharpness']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-sharpness-min-points needs --map-scans'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-sharpness-min-points', '5']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-sharpness-min-points must be >= 2'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-scans', str(tmp_path), '--out', str(tmp_path / 'o'), '--map-sharpness',
                              '--map-sharpness-min-points', '1']), emit=lines.append)
    assert lines == []  # found before anything is reported
    with pytest.raises(SystemExit, match='--map-sharpness needs --map-scans'):
        trajectory.main(['--features-root', str(pairs), '--map-sharpness'])


def test_sharpness_line_format():
    line = trajectory.sharpness_line(5, 'chained', 4, dict(voxels=100, qualified=40, degenerate=2, plane_thickness=0.0085, entropy=-6.25))
    assert line == 'seq 5 chained sharpness: 40 of 100 voxels with >= 4 points, plane thickness 8.500 mm, entropy -6.2500 (2 degenerate)'


# ---- the restatement on hand-worked voxels -----------------------------------------------------------------------------------

def at(cell, u, low=0):
    """The coordinate with the given cell, local coordinate u and `low` < 256 steps of 2^-22 m below u's resolution."""
    return np.float32(cell * V + u * S + low * 2.0 ** -22)


def rows(cells, us, lows=(0, 0, 0)):
    return np.float32([[at(c, u, l) for c, u, l in zip(cells, us, lows)]])


def test_local_coordinates_on_cell_faces_and_in_negative_cells():
    cloud = np.concatenate([rows((0, 1, -1), (0, 0, 0)),            # on the lower faces: u = 0 in cells 0, 1 and -1
                            rows((0, 1, -1), (4095, 4095, 4095)),  # the last step of the same cells
                            rows((0, 1, -1), (4095, 4095, 4095), (255, 255, 255)),  # ... and its last 2^-22: still 4095, not the next cell
                            rows((-1, -3, 2), (0, 0, 0), (1, 1, 1)),   # just above a face
                            rows((-2, -2, -2), (1, 2048, 4094), (7, 0, 200))])
    key, q, skipped = VM.quantise(cloud, EYE, V, 3)
    assert len(key) == 5 and not any(skipped.values())
    assert (q[:, :3] >> 20).tolist() == [[0, 1, -1], [0, 1, -1], [0, 1, -1], [-1, -3, 2], [-2, -2, -2]]
    u = MR.local(q)
    assert u.tolist() == [[0, 0, 0], [4095, 4095, 4095], [4095, 4095, 4095], [0, 0, 0], [1, 2048, 4094]]
    assert u.min() >= 0 and u.max() < 4096
    nine = MR.nine(u)
    assert nine[4].tolist() == [1, 2048, 4094, 1, 2048, 4094, 2048 * 2048, 2048 * 4094, 4094 * 4094]
    # one step below a face is the cell below, from either side of zero
    cloud = np.float32([[at(1, 0) - np.float32(2.0 ** -22), at(0, 0) - np.float32(2.0 ** -22), at(-1, 0) - np.float32(2.0 ** -22)]])
    _, q, _ = VM.quantise(cloud, EYE, V, 3)
    assert (q[:, :3] >> 20).tolist() == [[0, -1, -2]] and MR.local(q).tolist() == [[4095, 4095, 4095]]


def test_a_single_point_has_zero_covariance():
    for cells in ((0, 0, 0), (-5, 3, -1)):
        m = MR.build([rows(cells, (17, 4095, 1000), (3, 0, 255))], [EYE], V, channels=3)
        sums, cov, w, normal = m.extract()
        assert sums.tolist() == [[17, 4095, 1000, 17 * 17, 17 * 4095, 17 * 1000, 4095 * 4095, 4095 * 1000, 1000 * 1000]]
        assert (cov == 0).all() and (w == 0).all() and abs(np.linalg.norm(normal[0]) - 1) < 1e-15
        r = m.sharpness(1)
        assert (r['voxels'], r['qualified'], r['degenerate'], r['plane_thickness']) == (1, 1, 1, 0.0) and np.isnan(r['entropy'])
        assert m.sharpness(4)['qualified'] == 0 and np.isnan(m.sharpness(4)['plane_thickness'])


def test_two_points():
    # u = (0, 100, 10) and (4095, 100, 30): mean x 2047.5, variance 2047.5^2; z: mean 20, variance 100; cov xz = 2047.5 * 10
    cloud = np.concatenate([rows((-1, 2, 0), (0, 100, 10)), rows((-1, 2, 0), (4095, 100, 30), (9, 9, 9))])
    sums, cov, w, normal = MR.build([cloud], [EYE], V, channels=3).extract()
    assert sums.tolist() == [[4095, 200, 40, 4095 * 4095, 409500, 4095 * 30, 20000, 4000, 1000]]
    assert cov.tolist() == [[2047.5 ** 2 * S * S, 0.0, 20475.0 * S * S, 0.0, 0.0, 100.0 * S * S]]
    # rank one: the two small eigenvalues are zero up to rounding, the large one is the squared half distance
    half2 = (2047.5 ** 2 + 100.0) * S * S
    assert abs(w[0, 2] - half2) < 1e-15 * half2 * 8 and np.abs(w[0, :2]).max() < 1e-15 * half2 * 8


def test_the_corners_of_a_cube():
    # u in {1000, 3000}^3 in cell (-2, 0, 1): mean 2000, every variance 1000^2, every covariance 0, in steps of 2^-14 m
    corners = [(a, b, c) for a in (1000, 3000) for b in (1000, 3000) for c in (1000, 3000)]
    cloud = np.concatenate([rows((-2, 0, 1), u) for u in corners])
    m = MR.build([cloud[:3], cloud[3:]], [EYE, EYE], V, channels=3)
    sums, cov, w, normal = m.extract()
    assert len(sums) == 1 and sums[0, :3].tolist() == [16000] * 3 and sums[0, 3] == 4 * (1000 ** 2 + 3000 ** 2) and sums[0, 4] == 8 * 2000 ** 2
    var = 1.0e6 * S * S
    assert cov.tolist() == [[var, 0.0, 0.0, var, 0.0, var]]
    assert w.tolist() == [[var, var, var]]
    r = m.sharpness(4)
    assert (r['voxels'], r['qualified'], r['degenerate']) == (1, 1, 0) and r['plane_thickness'] == np.sqrt(var)
    assert abs(r['entropy'] - 0.5 * np.log((2 * np.pi * np.e * var) ** 3)) < 1e-12
    # the moments depend on the set of points only
    again = MR.build([cloud[::-1]], [EYE], V, channels=3).extract()
    assert all(np.array_equal(a, b) for a, b in zip(again[:2], (sums, cov)))


def test_sign_rule_and_plane_normal():
    assert MR.signed([[-0.6, 0.0, 0.8], [0.6, 0.0, -0.8], [-0.5, 0.5, 0.1], [0.5, -0.5, 0.1], [0.0, -1.0, 0.0]]).tolist() == \
        [[-0.6, 0.0, 0.8], [-0.6, 0.0, 0.8], [0.5, -0.5, -0.1], [0.5, -0.5, 0.1], [0.0, 1.0, 0.0]]
    # the plane u_z = u_x in one voxel: normal (1, 0, -1) / sqrt 2 by the sign rule (a tie between x and z: the lowest axis decides)
    grid = [(a, b, a) for a in range(0, 4096, 512) for b in range(0, 4096, 512)]
    cloud = np.concatenate([rows((0, 0, 0), u) for u in grid])
    _, cov, w, normal = MR.build([cloud], [EYE], V, channels=3).extract()
    assert abs(w[0, 0]) < 1e-18 and w[0, 1] > 1e-4 * S  # flat
    assert np.abs(np.abs(normal[0]) - np.array([1, 0, 1]) / np.sqrt(2)).max() < 1e-12 and normal[0, 0] * normal[0, 2] < 0


# ---- what the moments are for ------------------------------------------------------------------------------------------------

def ground_and_walls(rng, n_scans=8, per_scan=6000, range_noise=0.02):
    """A ground plane (z = 0, 36 m x 16 m) and two walls (y = +-8 m, 4 m high) seen from n_scans poses 3 m apart along x, 1.7 m
    above the ground: every scan samples the surfaces within 25 m, moves each sample along its ray by N(0, range_noise) and stores it
    in the sensor frame.  -> (clouds float32 [per_scan, 3], true poses [n, 4, 4])."""
    clouds, poses = [], []
    for k in range(n_scans):
        yaw = 0.05 * np.sin(k)
        X = np.eye(4)
        X[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        X[:3, 3] = [6.0 + 3.0 * k, 0.3 * np.cos(k), 1.7]
        n_g = per_scan * 6 // 10
        n_w = (per_scan - n_g) // 2
        ground = np.stack([rng.uniform(0, 36, n_g), rng.uniform(-8, 8, n_g), np.zeros(n_g)], 1)
        walls = [np.stack([rng.uniform(0, 36, n_w), np.full(n_w, y), rng.uniform(0, 4, n_w)], 1) for y in (-8.0, 8.0)]
        world = np.concatenate([ground] + walls)
        ray = world - X[:3, 3]
        dist = np.linalg.norm(ray, axis=1, keepdims=True)
        world = X[:3, 3] + ray * (1.0 + rng.normal(0.0, range_noise, dist.shape) / dist)
        world = world[dist[:, 0] < 25.0]
        inv = np.linalg.inv(X)
        clouds.append((world @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        poses.append(X)
    return clouds, np.stack(poses)


def perturbed(poses, rng, sigma_t, sigma_r):
    out = poses.copy()
    for X in out:
        w = rng.normal(0.0, sigma_r, 3)
        th = np.linalg.norm(w)
        if th > 0:
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
            X[:3, :3] = X[:3, :3] @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
        X[:3, 3] += rng.normal(0.0, sigma_t, 3)
    return out


def test_plane_thickness_grows_with_the_pose_noise():
    rng = np.random.default_rng(2024)
    clouds, poses = ground_and_walls(rng)
    levels = ((0.0, 0.0), (0.02, 0.002), (0.05, 0.005))
    reports = [MR.build(clouds, perturbed(poses, np.random.default_rng(7), t, r), 0.3, channels=3).sharpness(4) for t, r in levels]
    for (t, r), rep in zip(levels, reports):
        print(f"pose noise {t * 100:g} cm / {r:g} rad: {rep['voxels']} voxels, {rep['qualified']} with >= 4 points, plane thickness "
              f"{rep['plane_thickness'] * 1e3:.2f} mm, entropy {rep['entropy']:.3f}, {rep['degenerate']} degenerate")
    thick = [rep['plane_thickness'] for rep in reports]
    assert thick[0] < thick[1] < thick[2]
    assert all(rep['qualified'] > 1000 for rep in reports)
    # without pose noise a surface inside a voxel is about as thick as the range noise lets it be (2 cm along rays that meet the
    # ground at a grazing angle: well below 2 cm across it), never thicker than the voxel's own spread 0.3 / sqrt 12
    assert 0.002 < thick[0] < 0.02 and thick[2] < 0.3 / np.sqrt(12.0)
