"""CPU: the per-point queries' declarations and bindings, the `--map-clean` options of `python -m rdmnet_amd.trajectory` that need no
GPU, and the NumPy restatement tests/voxel_query_restatement.py itself: its distances against the registration's cost, and what the
queries are for -- a car that moves through a street is transient in the map that holds it and off the surface of a map that does not.

The scene (`scene`): test_voxel_register.street (4000 points a scan, 8 scans) and, after the street's rows of scan k, 150 points on the
five visible faces of a 3 x 1.6 x 1.15 m box that stands on z in [0.35, 1.5] at x = 6 + 4 k, y = 2: it moves 4 m per scan."""
import os
import re

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_observations_restatement as OR
import voxel_query_restatement as QR
import voxel_register_restatement as RR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs
from test_voxel_register import street

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
CAR = 150
_cache = {}


def car(rng, k, n=CAR):
    """n world points on the top and the four sides of the box of scan k, each face with a share of the points that is its area's."""
    size, lo = np.array([3.0, 1.6, 1.15]), np.array([6.0 + 4.0 * k - 1.5, 2.0 - 0.8, 0.35])
    faces = [(2, 1), (0, 0), (0, 1), (1, 0), (1, 1)]  # (axis, 0 = low side or 1 = high side): top, -x, +x, -y, +y
    area = np.array([size[(a + 1) % 3] * size[(a + 2) % 3] for a, _ in faces])
    which = rng.choice(len(faces), n, p=area / area.sum())
    p = lo + rng.uniform(0.0, 1.0, (n, 3)) * size
    for j, (a, side) in enumerate(faces):
        p[which == j, a] = lo[a] + side * size[a]
    return p


def scene(seed):
    """-> (street clouds, car clouds, the scans = street rows then car rows, poses); computed once per seed, never changed."""
    if seed not in _cache:
        rng = np.random.default_rng(seed)
        streets, poses = street(rng, 8, 4000)
        cars = []
        for k, X in enumerate(poses):
            inv = np.linalg.inv(X)
            cars.append((car(rng, k) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        _cache[seed] = (streets, cars, [np.concatenate([s, c]) for s, c in zip(streets, cars)], poses)
    return _cache[seed]


def maps(clouds, poses, voxel):
    return MR.build(clouds, poses, voxel, 3), OR.build(clouds, poses, voxel, 3)


def test_header_declares_the_entry_point_and_the_labels_and_bindings_have_them():
    text = open(HEADER).read()
    name = 'rdm_voxel_map_query'
    decl = re.search(r'^int ' + name + r'\(([^;]*)\);', text, re.M).group(1)
    assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()])
    for code, label in enumerate(_lib.VOXEL_POINT_LABELS):
        assert re.search(r'#define RDM_VOXEL_POINT_%s %d\b' % (label.upper(), code), text), label
    assert _lib.VOXEL_POINT_LABELS == QR.LABELS and len(QR.LABELS) == 7
    assert re.search(r'#define RDM_VOXEL_QUERY_TALLIES %d\b' % _lib.VOXEL_QUERY_TALLIES, text) and _lib.VOXEL_QUERY_TALLIES == 8
    assert 'tests/voxel_query_restatement.py' in text
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)  # a new entry point does not bump it
    # the map's head, then the two optional blocks, the voxel and integrate's batch, as rdm_voxel_map_register has them
    sig, reg = _lib.SIGNATURES[name][1], _lib.SIGNATURES['rdm_voxel_map_register'][1]
    assert sig[:6] == reg[:6] and sig[6:8] == [_lib.c_void, _lib.c_size] and sig[8:19] == reg[6:17]
    assert 'observations' in decl and 'tallies' in decl


@pytest.mark.parametrize('voxel', [0.3, 1.0])
@pytest.mark.parametrize('neighbors', [1, 7])
def test_the_rows_distances_add_up_to_the_registrations_cost(voxel, neighbors):
    streets, _, scans, poses = scene(5)
    table, observed = maps(scans[:4] + scans[5:], np.concatenate([poses[:4], poses[5:]]), voxel)
    X = RR.apply(poses[4], np.array([0.002, -0.001, 0.003, 0.03, -0.02, 0.01]))
    for min_points in (1, 4):
        q = QR.query(table, observed, scans[4], X, sigma=0.02, min_points=min_points, neighbors=neighbors)
        e = RR.evaluate(table, scans[4], X, sigma=0.02, min_points=min_points, neighbors=neighbors)
        assert abs(q['d2_sum'].sum() - e['cost']) <= 1e-12 * abs(e['cost']) and e['cost'] > 0
        assert int(q['pairs'].sum()) == e['n_corr'] > 0
        assert q['abs_sum'].sum() >= e['abs_cost'] * (1 - 1e-12)  # (nine terms a pair against the registration's one)
        has = q['best'] >= 0
        assert (q['d2'][has] <= q['each'][has].min(1)).all() and np.isinf(q['d2'][~has]).all() and (q['pairs'][~has] == 0).all()
        assert (q['d2_sum'] >= q['d2'] * (1 - 1e-15))[has].all() and (q['labels'][~has] == QR.UNMAPPED).all()


@pytest.mark.parametrize('seed', [5, 7])
def test_a_moving_car_is_transient_in_its_own_map_and_off_the_surface_of_a_prior_map(seed):
    streets, cars, scans, poses = scene(seed)
    n_street = sum(len(s) for s in streets)
    is_car = np.concatenate([np.arange(len(s)) >= len(s) - CAR for s in scans])
    assert is_car.sum() == 8 * CAR
    # the map of all eight scans, car included, at 0.3 m: the scan count finds the car
    q = QR.batch(*maps(scans, poses, 0.3), scans, poses, min_scans=2)
    lab = q['labels']
    print(f'seed {seed}, own map at 0.3 m, min_scans 2: car {np.bincount(lab[is_car], minlength=7).tolist()}, street '
          f'{np.bincount(lab[~is_car], minlength=7).tolist()} of {n_street} (labels {QR.LABELS})')
    assert (lab[is_car] == QR.TRANSIENT).all()
    assert (lab[~is_car] == QR.STATIC).sum() > (lab[~is_car] == QR.TRANSIENT).sum() > 0
    # ... at 1 m it does not: car points share a voxel with the ground
    coarse = QR.batch(*maps(scans, poses, 1.0), scans, poses, min_scans=2)['labels']
    print(f'seed {seed}, own map at 1 m, min_scans 2: car {np.bincount(coarse[is_car], minlength=7).tolist()}')
    # the street-only map of the same eight scans (a prior map) at 1 m: the distance finds what the count cannot
    q = QR.batch(*maps(streets, poses, 1.0), scans, poses, max_d2=25.0)
    lab = q['labels']
    print(f'seed {seed}, prior map at 1 m, max_d2 25: car {np.bincount(lab[is_car], minlength=7).tolist()}, street '
          f'{np.bincount(lab[~is_car], minlength=7).tolist()}')
    assert (lab[is_car] != QR.STATIC).all() and set(lab[is_car].tolist()) <= {QR.UNMAPPED, QR.OFF_SURFACE}
    assert (lab[~is_car] == QR.STATIC).all()
    assert q['tallies'].shape == (8, 8) and q['tallies'][:, :7].sum() == len(lab) and q['tallies'][:, 7].sum() == q['pairs'].sum()


def test_gates_and_precedence_on_a_handful_of_rows():
    cloud = np.array([[0.2, 0.2, 0.2], [0.25, 0.2, 0.2], [np.nan, 0, 0], [50.0, 0, 0], [0.5, 0.5, 3.5e6], [5.5, 0.5, 0.5], [0.2, 0.2, 0.6],
                      [2.5, 0.5, 0.5]], np.float32)
    X = [np.eye(4)] * 2
    built = [cloud[[0, 1, 7]], cloud[[0, 7]] + np.float32(0.01)]  # voxel (0,0,0) in two scans, three points near one place; (2,0,0) two points
    table, observed = maps(built, X, 1.0)
    q = QR.query(table, observed, cloud, np.eye(4), sigma=0.02, min_points=1, neighbors=1, min_scans=2, max_d2=25.0)
    assert q['labels'].tolist() == [QR.STATIC, QR.STATIC, QR.NONFINITE, QR.UNMAPPED, QR.EXTENT, QR.UNMAPPED, QR.OFF_SURFACE, QR.STATIC]
    q = QR.query(table, observed, cloud, np.eye(4), min_scans=3, max_d2=25.0, max_range=40.0)
    assert q['labels'].tolist() == [QR.TRANSIENT, QR.TRANSIENT, QR.NONFINITE, QR.RANGE, QR.RANGE, QR.UNMAPPED, QR.TRANSIENT, QR.TRANSIENT]
    q = QR.query(table, observed, cloud, np.eye(4), min_points=3, max_d2=25.0, max_range=60.0)
    assert q['labels'][7] == QR.UNMAPPED and q['counts'].tolist() == [3, 3, 0, 0, 0, 0, 3, 0]
    assert q['scans'].tolist()[:2] == [2, 2] and q['first'][0] == 0 and q['last'][0] == 1 and q['first'][2] == OR.MAX_ID and q['last'][2] == -1
    q7 = QR.query(table, observed, cloud, np.eye(4), neighbors=7, max_range=60.0)
    assert q7['best'].tolist() == [0, 0, -1, -1, -1, -1, 0, 0] and q7['pairs'].tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    near = QR.query(table, observed, np.array([[1.5, 0.5, 0.5]], np.float32), np.eye(4), neighbors=7)
    assert near['pairs'].tolist() == [2] and near['best'][0] in (1, 2) and near['d2'][0] == near['each'][0].min()
    flat = QR.query(table, None, cloud[:1], np.eye(4), sigma=0.5, moments=False)
    mu = table.map.sums[0, :3] / table.map.counts[0] / QR.VM.SCALE
    assert abs(flat['d2'][0] - ((cloud[0].astype(np.float64) - mu) ** 2).sum() / 0.25) < 1e-12


# ---- the command line ------------------------------------------------------------------------------------------------------------

def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_clean_options_parse_and_need_map_scans_out_and_a_criterion(tmp_path):
    a = parse(['--features-root', 'x'])
    assert a.map_clean is False and (a.map_clean_max_d2, a.map_clean_sigma, a.map_clean_neighbors) == (np.inf, 0.02, 1)
    a = parse(['--features-root', 'x', '--map-scans', 'R', '--out', 'o', '--map-clean', '--map-clean-max-d2', '25', '--map-clean-sigma', '0.05',
               '--map-clean-neighbors', '7'])
    assert a.map_clean is True and (a.map_clean_max_d2, a.map_clean_sigma, a.map_clean_neighbors) == (25.0, 0.05, 7)
    with pytest.raises(SystemExit):
        parse(['--features-root', 'x', '--map-clean-neighbors', '3'])
    pairs = tmp_path / 'pairs'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    lines = []
    base = ['--features-root', str(pairs)]
    full = base + ['--map-scans', str(tmp_path), '--out', str(tmp_path / 'o')]
    for argv in (base + ['--map-clean'], base + ['--map-clean', '--map-scans', str(tmp_path)], base + ['--map-clean', '--out', str(tmp_path / 'o')]):
        with pytest.raises(trajectory.TrajectoryError, match='--map-clean needs --map-scans and --out'):
            trajectory.run(parse(argv + ['--map-min-scans', '2']), emit=lines.append)
    for flag, value in (('--map-clean-max-d2', '25'), ('--map-clean-sigma', '0.1'), ('--map-clean-neighbors', '7')):
        with pytest.raises(trajectory.TrajectoryError, match=flag + ' needs --map-clean'):
            trajectory.run(parse(full + [flag, value]), emit=lines.append)
    for extra in ([], ['--map-min-scans', '1'], ['--map-clean-sigma', '0.1']):
        with pytest.raises(trajectory.TrajectoryError, match='--map-clean needs a criterion'):
            trajectory.run(parse(full + ['--map-clean'] + extra), emit=lines.append)
    for flag, value in (('--map-clean-sigma', '0'), ('--map-clean-max-d2', '-1'), ('--map-clean-max-d2', 'nan')):
        with pytest.raises(trajectory.TrajectoryError, match='--map-clean-sigma must be > 0 and --map-clean-max-d2 >= 0'):
            trajectory.run(parse(full + ['--map-clean', '--map-min-scans', '2', flag, value]), emit=lines.append)
    assert lines == []  # found before anything is reported
    with pytest.raises(SystemExit, match='--map-clean needs --map-scans and --out'):
        trajectory.main(base + ['--map-clean'])


def test_clean_line_format():
    tallies = np.array([[1, 2, 3, 10, 20, 30, 100, 150], [0, 0, 1, 0, 5, 0, 50, 55]])
    assert trajectory.clean_line(3, 'chained', tallies, 2, 25.0) == (
        'seq 3 chained clean: 150 of 222 points kept in 2 scans, dropped: 10 unmapped, 25 transient (< 2 scans), 30 off surface (d2 > 25), '
        '7 gated')
    assert trajectory.clean_line(3, 'refined', tallies[:1], 2, np.inf).endswith('20 transient (< 2 scans), 30 off surface (d2 > inf), 6 gated')
