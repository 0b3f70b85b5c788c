"""CPU: the NumPy restatement of the voxel map (tests/voxel_map_restatement.py) against the properties its definition promises, and
the parts of `python -m rdmnet_amd.trajectory --map-scans` that need no GPU (option parsing, the TrajectoryError paths).

The means: a voxel's stored mean differs from the float64 mean of its points' world coordinates by less than voxel 2^-20 (every
coordinate is floored to a multiple of that step, so the mean of the floored values is below the true mean by less than one
step) plus the error of the float64 expressions (a few 2^-53 relative, at most 1e-12 m here) plus one fp32 rounding of the result;
an attribute by half a step (round to nearest) plus the fp32 rounding."""
import os

import numpy as np
import pytest

import voxel_map_restatement as VM
from rdmnet_amd import trajectory


FACES = (-0.3, -0.6, 0.0, 0.3)  # cell faces at 0.3 m


def random_pose(rng, t_max=500.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    X = np.eye(4)
    X[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    X[:3, 3] = rng.uniform(-t_max, t_max, 3)
    return X


def with_attribute(cloud, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([cloud, rng.random((len(cloud), 1), dtype=np.float32)], 1)


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_invariant_under_permutation_and_splitting(scans):
    rng = np.random.default_rng(0)
    clouds = [with_attribute(scans[k][:4000], i) for i, k in enumerate(('s000000', 's000004', 's000007'))]
    poses = [random_pose(rng) for _ in clouds]
    one = VM.build(clouds, poses, 0.3)
    ref = one.extract()
    assert len(ref[0]) > 1000 and ref[1].max() > 1
    shuffled = [c[rng.permutation(len(c))] for c in clouds]
    assert same(VM.build(shuffled[::-1], poses[::-1], 0.3).extract(), ref)
    split = VM.Map(0.3)
    for c, X in zip(clouds, poses):
        split.integrate([c[:1500]], [X])
        split.integrate([c[1500:], np.zeros((0, 4), np.float32)], [X, np.eye(4)])
    assert same(split.extract(), ref) and split.stats() == one.stats()
    assert one.stats()['integrated'] == sum(len(c) for c in clouds) == int(ref[1].sum())


def test_identity_pose_partitions_by_floor(scans):
    cloud = scans['s000000']
    for voxel in (0.3, 0.05):
        pts, counts, cells = VM.build([cloud], [np.eye(4)], voxel, channels=3).extract()
        want = np.floor(cloud.astype(np.float64) / voxel).astype(np.int64)
        uniq, n = np.unique(want, axis=0, return_counts=True)  # lexicographic = ascending key
        assert np.array_equal(cells, uniq) and np.array_equal(counts, n)
        assert (cells[:, 0].min() < 0) and (cells[:, 0].max() > 0)


def test_means_are_within_the_fixed_point_step_of_the_float64_means(scans):
    rng = np.random.default_rng(1)
    cloud, X, voxel = with_attribute(scans['s000004'], 5), random_pose(rng), 0.3
    pts, counts, cells = VM.build([cloud], [X], voxel).extract()
    world = cloud[:, :3].astype(np.float64) @ X[:3, :3].T + X[:3, 3]
    cell = np.floor(world / voxel).astype(np.int64)
    uniq, inverse, n = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    # (a point within 1e-9 m of a face could land on the other side under another association of the transform: none here)
    assert np.abs(world / voxel - np.round(world / voxel)).min() > 1e-8
    assert np.array_equal(uniq, cells) and np.array_equal(n, counts)
    mean = np.zeros((len(uniq), 4))
    np.add.at(mean, inverse, np.concatenate([world, cloud[:, 3:].astype(np.float64)], 1))
    mean /= n[:, None]
    err = np.abs(pts.astype(np.float64) - mean)
    ulp = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64)
    assert (err[:, :3] <= voxel * 2.0 ** -20 + 1e-12 + ulp[:, :3]).all()
    assert (err[:, 3] <= 2.0 ** -21 + ulp[:, 3]).all()
    assert (np.floor(pts[:, :3].astype(np.float64) / voxel) == cells).mean() > 0.99  # the means lie in their own cells


def test_points_on_a_cell_face_go_to_the_upper_cell():
    # world x exactly -0.3, -0.6, 0.0, 0.3 (float64, through the pose: the origin of four scans): w / 0.3 is exactly -1, -2, 0, 1,
    # and cell c covers [c voxel, (c + 1) voxel)
    origin = np.zeros((1, 3), np.float32)
    poses = []
    for t in FACES:
        X = np.eye(4)
        X[0, 3] = t
        poses.append(X)
    m = VM.build([origin] * 4, poses, 0.3, channels=3)
    pts, counts, cells = m.extract()
    assert cells.tolist() == [[-2, 0, 0], [-1, 0, 0], [0, 0, 0], [1, 0, 0]] and counts.tolist() == [1, 1, 1, 1]
    assert np.array_equal(pts[:, 0], np.float32([-0.6, -0.3, 0.0, 0.3]))  # the stored means are the faces themselves
    # the same figures as fp32 ROWS are not on the faces: float32(0.3) > 0.3 and float32(-0.3) < -0.3; the definition is floor(w /
    # voxel) of the values as given
    xs = np.float32(FACES)
    cloud = np.stack([xs, np.zeros(4, np.float32), np.zeros(4, np.float32)], 1)
    pts, counts, cells = VM.build([cloud], [np.eye(4)], 0.3, channels=3).extract()
    want = np.floor(xs.astype(np.float64) / 0.3).astype(np.int64)
    assert want.tolist() == [-2, -3, 0, 1]
    assert cells[:, 0].tolist() == sorted(want.tolist()) and (cells[:, 1:] == 0).all() and counts.tolist() == [1, 1, 1, 1]
    # exactly representable faces: 0.25 m voxels
    xs = np.float32([-0.25, -0.5, 0.0, 0.25, -1e-30])
    cloud = np.stack([np.zeros(5, np.float32), xs, np.zeros(5, np.float32)], 1)
    pts, counts, cells = VM.build([cloud], [np.eye(4)], 0.25, channels=3).extract()
    assert cells[:, 1].tolist() == [-2, -1, 0, 1] and counts.tolist() == [1, 2, 1, 1]


def test_range_gate_keeps_the_boundary():
    cloud = np.float32([[48, 64, 0], [48, 64, 0.01], [3, 4, 0], [3, 4, -0.01], [2.9, 4, 0], [np.nan, 1, 1], [1, np.inf, 1], [10, 0, 0]])
    m = VM.build([cloud], [np.eye(4)], 0.3, channels=3, min_range=5.0, max_range=80.0)
    assert m.stats() == dict(occupied=4, integrated=4, skipped_nonfinite=2, skipped_range=2, out_of_extent=0, dropped_full=0)
    assert VM.build([cloud], [np.eye(4)], 0.3, channels=3).stats()['integrated'] == 6  # the default is no gate
    # the gate is in the sensor frame: a pose far away changes nothing
    far = np.eye(4)
    far[:3, 3] = [400.0, -300.0, 20.0]
    assert VM.build([cloud], [far], 0.3, channels=3, min_range=5.0, max_range=80.0).stats()['integrated'] == 4


def test_extent_and_attribute_limits():
    cloud = np.float32([[1, 2, 3, 0.5], [1, 2, 3, 1048576.0], [1, 2, 3, -1048575.0], [3.2e5, 0, 0, 0], [0, 0, -314572.9, 0], [0, 0, 314572.7, 0]])
    m = VM.build([cloud], [np.eye(4)], 0.3)
    st = m.stats()
    assert (st['integrated'], st['out_of_extent']) == (3, 3)  # 2^20 cells of 0.3 m end at 314572.8 m
    pts, counts, cells = m.extract(min_points=2)
    assert counts.tolist() == [2] and cells.tolist() == [[3, 6, 10]] and pts[0, 3] == np.float32((0.5 - 1048575.0) / 2)


# ---- the command line (no GPU) ---------------------------------------------------------------------------------------------

def write_pairs(root, seq, frames):
    for a, b in zip(frames[:-1], frames[1:]):
        np.savez(os.path.join(root, f'{seq}_{a}_{b}.npz'), estimated_transform=np.eye(4), transform=np.eye(4), information=np.eye(6))


def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_map_options_parse_with_their_defaults(tmp_path):
    a = parse(['--features-root', str(tmp_path)])
    assert a.map_scans is None and not a.map_raw and a.map_voxel == 0.3 and a.map_min_points == 1 and a.map_range is None and a.map_batch == 64
    a = parse(['--features-root', 'x', '--map-scans', 'R', '--map-raw', '--map-voxel', '0.1', '--map-min-points', '3', '--map-range',
               '2', '60', '--map-batch', '8', '--out', 'o'])
    assert (a.map_scans, a.map_raw, a.map_voxel, a.map_min_points, a.map_range, a.map_batch) == ('R', True, 0.1, 3, [2.0, 60.0], 8)
    with pytest.raises(SystemExit):
        parse(['--features-root', 'x', '--map-range', '2'])


def test_map_scans_needs_out_and_names_a_missing_scan(tmp_path):
    pairs, data = tmp_path / 'pairs', tmp_path / 'data'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10, 20])
    folder = data / 'downsampled_xyzi' / '07'
    os.makedirs(folder)
    for f in (0, 20):
        np.save(folder / ('%06d.npy' % f), np.zeros((5, 4), np.float32))
    with pytest.raises(trajectory.TrajectoryError, match='--map-scans needs --out'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-scans', str(data)]), emit=lambda _: None)
    lines = []
    with pytest.raises(trajectory.TrajectoryError, match=r'downsampled_xyzi/07/000010\.npy: no such scan file'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(tmp_path / 'o')]), emit=lines.append)
    assert lines == []  # found before anything is reported or written
    with pytest.raises(trajectory.TrajectoryError, match=r'sequences/07/velodyne/000000\.bin: no such scan file'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-scans', str(data), '--map-raw', '--out', str(tmp_path / 'o')]),
                       emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-range'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-scans', str(data), '--map-range', '9', '3', '--out', str(tmp_path / 'o')]),
                       emit=lines.append)
    with pytest.raises(SystemExit, match='no such scan file'):
        trajectory.main(['--features-root', str(pairs), '--map-scans', str(data), '--out', str(tmp_path / 'o')])
    with pytest.raises(trajectory.TrajectoryError, match=r'nowhere\.npy: no such scan file'):
        trajectory.build_map([str(tmp_path / 'nowhere.npy')], [np.eye(4)])
