"""CPU: the voxel observations' declarations and bindings, the `--map-min-scans` / `--map-refine-min-scans` options of `python -m
rdmnet_amd.trajectory` that need no GPU, the NumPy restatement tests/voxel_observations_restatement.py on hand-worked cases, and what
the observations are for: a box that moves 4 m between the scans of a street leaves voxels that are seen in exactly one scan, the
street's own voxels are seen in many, and pruning at two scans removes the first and keeps the second.

The hand-worked cases use 1 m voxels and coordinates that are exact in float32, so every figure is compared with ==."""
import os
import re

import numpy as np
import pytest

import voxel_map_restatement as VM
import voxel_observations_restatement as OR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs
from test_voxel_register import street

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
NEW = ('rdm_voxel_observations_bytes', 'rdm_voxel_observations_reset', 'rdm_voxel_map_integrate_observed', 'rdm_voxel_observations_rehash',
       'rdm_voxel_map_extract_observations', 'rdm_voxel_map_prune')
EYE = np.eye(4)


def test_header_declares_the_entry_points_and_bindings_have_them():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r'^(?:size_t|int) ' + name + r'\(([^;]*)\);', text, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()]), name
    assert re.search(r'#define RDM_VOXEL_OBSERVATIONS_MAX_SCANS 64\b', text)
    assert _lib.VOXEL_OBSERVATIONS_MAX_SCANS == OR.MAX_SCANS == 64 == trajectory.MAP_DEFAULTS['batch']
    assert 'tests/voxel_observations_restatement.py' in text
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)  # new entry points do not bump it
    # the integrate with observations takes the integrate with moments' arguments plus the block (pointer, bytes) and first_id
    with_moments, observed = _lib.SIGNATURES['rdm_voxel_map_integrate_moments'][1], _lib.SIGNATURES['rdm_voxel_map_integrate_observed'][1]
    assert observed == with_moments[:-1] + [_lib.c_void, _lib.c_size, _lib.c_i64] + with_moments[-1:]
    # both extracts and both rehashes are driven alike
    assert _lib.SIGNATURES['rdm_voxel_observations_rehash'] == _lib.SIGNATURES['rdm_voxel_moments_rehash']
    a, b = _lib.SIGNATURES['rdm_voxel_map_extract_observations'][1], _lib.SIGNATURES['rdm_voxel_map_extract_moments'][1]
    assert a[:8] == b[:8] and a[-6:] == b[-6:] and len(a) == len(b) - 1  # (three outputs for four)


def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_min_scans_options_parse_and_need_their_flags(tmp_path):
    a = parse(['--features-root', 'x'])
    assert (a.map_min_scans, a.map_refine_min_scans) == (1, 1)
    a = parse(['--features-root', 'x', '--map-scans', 'R', '--out', 'o', '--map-min-scans', '2', '--map-refine', '--map-refine-min-scans', '3'])
    assert (a.map_min_scans, a.map_refine_min_scans) == (2, 3)
    pairs = tmp_path / 'pairs'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    lines = []
    base = ['--features-root', str(pairs)]
    with_map = base + ['--map-scans', str(tmp_path), '--out', str(tmp_path / 'o')]
    with pytest.raises(trajectory.TrajectoryError, match='--map-min-scans needs --map-scans'):
        trajectory.run(parse(base + ['--map-min-scans', '2']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine-min-scans needs --map-refine'):
        trajectory.run(parse(with_map + ['--map-refine-min-scans', '2']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-min-scans must be >= 1'):
        trajectory.run(parse(with_map + ['--map-min-scans', '0']), emit=lines.append)
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine-min-scans must be >= 1'):
        trajectory.run(parse(with_map + ['--map-refine', '--map-refine-min-scans', '0']), emit=lines.append)
    assert lines == []  # found before anything is reported
    with pytest.raises(SystemExit, match='--map-min-scans needs --map-scans'):
        trajectory.main(base + ['--map-min-scans', '2'])
    # the defaults are no request: a run without maps stays a run without maps
    trajectory.run(parse(base + ['--map-min-scans', '1']), emit=lines.append)
    assert len(lines) == 1 and ' chained: ' in lines[0]


def test_persistent_line_format():
    line = trajectory.persistent_line(5, 'chained', 2, dict(occupied=2146, integrated=46000), dict(occupied=2210, integrated=51200), 8)
    assert line == 'seq 5 chained persistent: 2146 of 2210 voxels seen in >= 2 scans, 46000 of 51200 points, 8 scans'


# ---- the restatement on hand-worked cases ------------------------------------------------------------------------------------

def rows(*xyz):
    return np.float32(xyz).reshape(-1, 3)


def table(m, min_points=1):
    """{cell: (count, scans, first, last)}."""
    _, counts, cells = m.map.extract(min_points)
    return {tuple(c): (int(n), int(s), int(a), int(b)) for c, n, s, a, b in zip(cells.tolist(), counts, *m.extract(min_points))}


def test_one_voxel_hit_by_two_scans():
    a = rows((0.5, 0.5, 0.5), (0.25, 0.75, 0.5), (2.5, 0.5, 0.5))  # two points in cell (0, 0, 0), one in (2, 0, 0)
    b = rows((0.125, 0.125, 0.875), (-0.5, 0.5, 0.5))              # one in (0, 0, 0), one in (-1, 0, 0)
    m = OR.build([a, b], [EYE, EYE], 1.0, channels=3)
    assert table(m) == {(-1, 0, 0): (1, 1, 1, 1), (0, 0, 0): (3, 2, 0, 1), (2, 0, 0): (1, 1, 0, 0)}
    assert m.num_scans == 2 and m.scans.dtype == np.int64 and all(v.dtype == np.int32 for v in m.extract())
    assert table(m, min_points=2) == {(0, 0, 0): (3, 2, 0, 1)}
    # many points of one scan are one observation; a point that the gate skips observes nothing
    m = OR.build([np.repeat(a[:1], 50, 0), rows((0.5, 0.5, np.nan), (0.5, 0.5, 0.25))[:1]], [EYE, EYE], 1.0, channels=3)
    assert table(m) == {(0, 0, 0): (50, 1, 0, 0)} and m.map.stats()['skipped_nonfinite'] == 1 and m.num_scans == 2
    # the same scan under another pose is another set of voxels: the pose belongs to the scan
    X = np.eye(4)
    X[0, 3] = 3.0
    assert table(OR.build([a[:1], a[:1]], [EYE, X], 1.0, channels=3)) == {(0, 0, 0): (1, 1, 0, 0), (3, 0, 0): (1, 1, 1, 1)}
    # pruning at two scans
    m = OR.build([a, b], [EYE, EYE], 1.0, channels=3)
    assert m.keep(2).tolist() == [False, True, False] and table(m.pruned(2)) == {(0, 0, 0): (3, 2, 0, 1)}
    assert m.pruned(2).map.stats() == dict(m.map.stats(), occupied=1, integrated=3)
    assert table(m.pruned(1, min_points=2)) == table(m.pruned(2)) and table(m.pruned(1)) == table(m) and table(m.pruned(3)) == {}


def test_ids_0_and_63_and_an_empty_scan_that_consumes_an_id():
    p, q = rows((0.5, 0.5, 0.5)), rows((5.5, 0.5, 0.5))
    empty = np.zeros((0, 3), np.float32)
    clouds = [p] + [q] * 62 + [p]
    m = OR.build(clouds, [EYE] * 64, 1.0, channels=3)
    assert table(m) == {(0, 0, 0): (2, 2, 0, 63), (5, 0, 0): (62, 62, 1, 62)} and m.num_scans == 64
    m = OR.build([p, empty, p], [EYE] * 3, 1.0, channels=3)
    assert table(m) == {(0, 0, 0): (2, 2, 0, 2)} and m.num_scans == 3
    m.integrate([empty], [EYE]).integrate([q], [EYE])
    assert table(m) == {(0, 0, 0): (2, 2, 0, 2), (5, 0, 0): (1, 1, 4, 4)} and m.num_scans == 5
    m.integrate([p], [EYE], first_id=OR.MAX_ID - 1)  # the largest id
    assert table(m)[(0, 0, 0)] == (3, 3, 0, OR.MAX_ID - 1)
    with pytest.raises(AssertionError):
        m.integrate([p], [EYE], first_id=OR.MAX_ID)


def test_batching_does_not_matter_under_fixed_ids():
    rng = np.random.default_rng(3)
    clouds = [rng.uniform(-2.0, 2.0, (40, 3)).astype(np.float32) for _ in range(5)]
    poses = [EYE] * 5
    whole = OR.build(clouds, poses, 1.0, channels=3)
    assert len(set(whole.scans.tolist())) > 2
    forms = [OR.Observed(1.0, 3).integrate(clouds[:2], poses[:2]).integrate(clouds[2:], poses[2:]),
             OR.Observed(1.0, 3).integrate(clouds[3:], poses[3:], first_id=3).integrate(clouds[:3], poses[:3], first_id=0)]
    single = OR.Observed(1.0, 3)
    for k in (4, 0, 2, 1, 3):
        single.integrate([clouds[k]], [EYE], first_id=k)
    for m in forms + [single]:
        assert table(m) == table(whole) and m.num_scans == 5
    # the rows of a scan in another order, and split scans under ONE id each are not a case: an id comes whole in one call


# ---- what the observations are for -------------------------------------------------------------------------------------------

def street_with_a_moving_box():
    """test_voxel_register.street under seed 5 and, drawn from the same generator after it, a box of 400 points per scan k with x uniform
    in [5 + 4 k, 6.5 + 4 k], y in [2.2, 3.8], z in [0.35, 1.55] (x, then y, then z, 400 values each), moved into the sensor frame by
    the scan's true pose.  -> (the street's clouds, the boxes, the poses)."""
    rng = np.random.default_rng(5)
    clouds, poses = street(rng)
    boxes = []
    for k, X in enumerate(poses):
        world = np.stack([rng.uniform(5.0 + 4.0 * k, 6.5 + 4.0 * k, 400), rng.uniform(2.2, 3.8, 400), rng.uniform(0.35, 1.55, 400)], 1)
        inv = np.linalg.inv(X)
        boxes.append((world @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    return clouds, boxes, poses


@pytest.mark.parametrize('voxel', [1.0, 0.3])
def test_a_moving_box_is_seen_once_and_the_street_many_times(voxel):
    clouds, boxes, poses = street_with_a_moving_box()
    static = OR.build(clouds, poses, voxel, channels=3)
    box = OR.build(boxes, poses, voxel, channels=3)
    both = OR.build([np.concatenate(cb) for cb in zip(clouds, boxes)], poses, voxel, channels=3)
    assert np.array_equal(both.map.keys, np.union1d(static.map.keys, box.map.keys))
    only_box = ~np.isin(both.map.keys, static.map.keys)
    untouched = ~np.isin(static.map.keys, box.map.keys)
    kept = both.keep(2)
    print(f'voxel {voxel:g} m: {len(static.map.keys)} static voxels, {(static.scans >= 2).mean() * 100:.1f} % seen in >= 2 scans; '
          f'{int(only_box.sum())} voxels hold only box points, {int((both.scans[only_box] == 1).sum())} of them seen in exactly one scan; '
          f'{int((~untouched).sum())} static voxels shared with the box')
    # every voxel that holds only box points is seen in exactly one scan and is not in the pruned map
    assert only_box.sum() > 0 and (both.scans[only_box] == 1).all() and not kept[only_box].any()
    pruned = both.pruned(2)
    assert not np.isin(pruned.map.keys, both.map.keys[only_box]).any() and np.array_equal(pruned.map.keys, both.map.keys[kept])
    # the box does not change what the street's voxels saw, wherever it does not touch them
    in_both = np.isin(both.map.keys, static.map.keys[untouched])
    for name in ('scans', 'first', 'last'):
        assert np.array_equal(getattr(both, name)[in_both], getattr(static, name)[untouched]), name
    assert np.array_equal(both.map.counts[in_both], static.map.counts[untouched])
    if voxel == 1.0:
        survive = np.isin(static.map.keys, pruned.map.keys).mean()
        assert survive >= 0.95, survive
