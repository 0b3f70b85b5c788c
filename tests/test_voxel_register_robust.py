"""CPU: the robust weights of the scan-to-map registration (rdm_voxel_map_register_robust, ops.VoxelMap.register(robust_scale=...),
`trajectory --map-refine-robust`): the declaration and its binding, the option, and the NumPy restatement
tests/voxel_register_robust_restatement.py itself -- off means the plain restatement, 2 g is the gradient of its weighted cost with
the associations held fixed, the weights sum to no more than the pairs -- and what the weights are for: a box that stands 0.3 m
further in the registered scan than in the map drags the plain registration by centimetres and the weighted one by millimetres, and
the sequential refinement of `--map-refine`, which a box moving 0.3 m per frame makes worse than its input, repairs the input.

Scans of 4 000 points plus the box, 1 m voxels, sigma 0.02, robust_scale 9, starts 5 cm / 5 mrad per axis off."""
import re

import numpy as np
import pytest

import voxel_moments_restatement as MR
import voxel_register_restatement as RR
import voxel_register_robust_restatement as WR
from rdmnet_amd import _lib, trajectory
from test_voxel_register import HEADER, perturb, pose_error

SCALE = 9.0
_cache = {}


def moved_box_scene(n_box):
    """Computed once, never changed: (clouds, true poses, the restatement's 1 m map of the seven scans that are not scan 4); the box
    of n_box points stands 0.3 m further in x and y in scan 4."""
    if n_box not in _cache:
        clouds, poses = WR.moved_box(np.random.default_rng(6), n_box)
        others = [k for k in range(len(clouds)) if k != 4]
        _cache[n_box] = (clouds, poses, MR.build([clouds[k] for k in others], poses[others], 1.0, 3))
    return _cache[n_box]


def test_header_declares_the_entry_point_and_the_binding_has_it():
    text = open(HEADER).read()
    name = 'rdm_voxel_map_register_robust'
    assert name in _lib.SIGNATURES
    decl = re.search(r'^int ' + name + r'\(([^;]*)\);', text, re.M).group(1)
    args = [a.strip() for a in decl.split(',') if a.strip()]
    sig, plain = _lib.SIGNATURES[name][1], _lib.SIGNATURES['rdm_voxel_map_register'][1]
    assert len(sig) == len(args) == len(plain) + 2
    # rdm_voxel_map_register's arguments in its order, robust_scale after trans_eps and weight_sums after costs
    assert args[20] == 'double trans_eps' and args[21] == 'double robust_scale' and sig[21] is _lib.ctypes.c_double
    assert args[25] == 'double* costs' and args[26] == 'double* weight_sums' and sig[26] is _lib.c_void
    assert sig[:21] == plain[:21] and sig[22:26] == plain[21:25] and sig[27:] == plain[25:]
    assert 'tests/voxel_register_robust_restatement.py' in text
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)
    assert not re.search(r'rdm_voxel_map_register_robust_workspace_bytes', text)  # the workspace is the plain form's


def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_the_option_parses_defaults_to_off_and_rejects_what_is_not_a_positive_number(tmp_path):
    assert parse(['--features-root', 'x']).map_refine_robust is None
    assert parse(['--features-root', 'x', '--map-refine', '--map-refine-robust', '9']).map_refine_robust == 9.0
    assert parse(['--features-root', 'x', '--map-localize', '--map-refine-robust', '2.5']).map_refine_robust == 2.5
    for bad in ('0', '-1', '-0.5', 'nine', 'nan', 'inf'):
        with pytest.raises(SystemExit):
            parse(['--features-root', 'x', '--map-refine', '--map-refine-robust', bad])
    from test_voxel_map import write_pairs
    pairs = tmp_path / 'pairs'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    lines = []
    with pytest.raises(trajectory.TrajectoryError, match='--map-refine-robust needs --map-refine'):
        trajectory.run(parse(['--features-root', str(pairs), '--map-refine-robust', '9']), emit=lines.append)
    assert lines == []


def test_robust_line_format():
    stats = dict(frames=5, iterations=np.array([0, 4, 6, 5, 5]), correspondences=np.array([0, 100, 200, 300, 400]), degenerate=0,
                 weights=np.array([0.0, 90.5, 150.25, 250.0, 309.25]))
    assert trajectory.robust_line(3, 'refined', 9.0, stats) == 'seq 3 refined robust weights: scale 9, 200.0 of 250 correspondences per frame by weight'
    assert trajectory.robust_line(3, 'localized', 2.5, stats) == ('seq 3 localized robust weights: scale 2.5, 160.0 of 200 correspondences per '
                                                                  'frame by weight')


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def test_off_is_the_plain_restatement():
    clouds, poses, table = moved_box_scene(400)
    X = perturb(poses[4], np.random.default_rng(3), 0.05, 0.005)
    for neighbors in (1, 7):
        a, b = WR.evaluate(table, clouds[4], X, neighbors=neighbors, terms=True), RR.evaluate(table, clouds[4], X, neighbors=neighbors, terms=True)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    a, b = WR.register(table, clouds[4], X, max_iteration=3), RR.register(table, clouds[4], X, max_iteration=3)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_twice_g_is_the_gradient_of_the_weighted_cost_with_the_associations_held_fixed():
    """The scene of test_voxel_register's quadratic test (points in the middle half of their voxels, so a small delta changes no
    association), with a tenth of the scan moved by up to 0.15 m per axis: the weights run from below a half to nearly one.
    rho(d2) = mu d2 / (mu + d2) has rho' = (mu / (mu + d2))^2 = l, hence d cost = sum l d(d2) = sum l 2 (J^T M r).delta = 2 g.delta:
    the central difference (cost(+delta) - cost(-delta)) / 2 is 2 g.delta up to the third order.  That order is at most
    |delta|^3 / 6 times the third derivative of the cost along delta; with |rho'| <= 1, |rho''| d2 <= 1/2 and |rho'''| d2^2 <= 1 it is
    bounded by a small multiple of the plain form's cubic term, 12 trace(H_plain's rotation block) |delta|^3 (test_voxel_register),
    taken here times 4."""
    rng = np.random.default_rng(4)
    cells = np.array([(a, b, c) for a in range(-3, 3) for b in range(-2, 2) for c in range(-1, 2)])
    world = np.concatenate([cells + rng.uniform(0.3, 0.7, (len(cells), 3)) for _ in range(8)]) + np.array([500.0, -300.0, 20.0])
    table = MR.build([world.astype(np.float32)], [np.eye(4)], 1.0, 3)
    X = perturb(np.eye(4), rng, 0.3, 0.5)
    X[:3, 3] += [500.0, -300.0, 20.0]
    inv = np.linalg.inv(X)
    seen = world[::2] + rng.normal(0, 0.03, world[::2].shape)
    far = rng.random(len(seen)) < 0.1
    seen[far] += rng.uniform(-0.15, 0.15, (int(far.sum()), 3))  # (still inside the voxel: from [0.3, 0.7] to [0.15, 0.85] less the noise)
    scan = (seen @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    for neighbors in (1, 7):
        e = WR.evaluate(table, scan, X, sigma=0.05, neighbors=neighbors, robust_scale=SCALE, terms=True)
        plain = RR.evaluate(table, scan, X, sigma=0.05, neighbors=neighbors)
        assert e['n_corr'] == plain['n_corr'] >= len(scan) and 0.0 < e['weight_sum'] <= e['n_corr']
        assert e['l'].min() < 0.5 and e['l'].max() > 0.9  # weights near one and weights that count for less than half
        assert np.abs(e['H'] - e['H'].T).max() <= 1e-9 * np.abs(e['H']).max()
        cubic = 4.0 * 12.0 * np.trace(plain['H'][:3, :3])
        for scale in (1e-3, 1e-4):
            for kind in ('both', 'both', 'rotation', 'translation'):
                delta = rng.normal(0, 1, 6)
                if kind != 'both':
                    delta[3 if kind == 'rotation' else 0:][:3] = 0.0
                delta *= scale / np.linalg.norm(delta)
                up = WR.evaluate(table, scan, RR.apply(X, delta), sigma=0.05, neighbors=neighbors, robust_scale=SCALE)
                down = WR.evaluate(table, scan, RR.apply(X, -delta), sigma=0.05, neighbors=neighbors, robust_scale=SCALE)
                assert up['n_corr'] == down['n_corr'] == e['n_corr']
                got, want = (up['cost'] - down['cost']) / 2.0, 2.0 * e['g'] @ delta
                bound = cubic * scale ** 3 + 1e-12 * e['abs_cost']
                print(f'neighbors {neighbors}, |delta| {scale:g} ({kind}): {got:.6e} against {want:.6e}, difference {got - want:.2e} (bound {bound:.2e})')
                assert abs(got - want) <= bound, (neighbors, scale, kind)
                # at the smaller step the check can tell the gradient, and the plain form's is another: it can tell the weights
                assert scale > 1e-4 or (abs(want) > 10 * bound and abs(2.0 * plain['g'] @ delta - want) > 10 * bound)


def test_weight_sum_is_at_most_the_pairs_and_a_huge_scale_is_the_plain_form():
    clouds, poses, table = moved_box_scene(400)
    for neighbors in (1, 7):
        e = WR.evaluate(table, clouds[4], poses[4], neighbors=neighbors, robust_scale=SCALE)
        plain = RR.evaluate(table, clouds[4], poses[4], neighbors=neighbors)
        assert e['n_corr'] == plain['n_corr'] and e['n_points'] == plain['n_points']
        assert 0.0 < e['weight_sum'] <= e['n_corr'] and e['cost'] <= plain['cost']
        huge = WR.evaluate(table, clouds[4], poses[4], neighbors=neighbors, robust_scale=1e30)
        assert huge['weight_sum'] == huge['n_corr']
        assert np.allclose(huge['H'], plain['H'], rtol=1e-12, atol=0.0) and np.isclose(huge['cost'], plain['cost'], rtol=1e-12, atol=0.0)


# ---- what the weights are for ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('neighbors', (1, 7))
@pytest.mark.parametrize('n_box', (400, 1200))
def test_a_box_that_stands_elsewhere_in_the_scan_than_in_the_map(n_box, neighbors):
    """The weighted translation error and the weighted rotation error are each below a third of the plain ones.  With these seeds
    the restatement's ratios are 15.5 / 21.1 (400, 1), 76 / 134 (400, 7), 14.3 / 34.1 (1 200, 1) and 45 / 112 (1 200, 7): plain 2.8,
    6.1, 6.5 and 11.4 cm, weighted 0.18, 0.08, 0.45 and 0.25 cm."""
    clouds, poses, table = moved_box_scene(n_box)
    X0 = perturb(poses[4], np.random.default_rng(3), 0.05, 0.005)
    plain = WR.register(table, clouds[4], X0, neighbors=neighbors)
    weighted = WR.register(table, clouds[4], X0, neighbors=neighbors, robust_scale=SCALE)
    a, b = pose_error(plain['transform'], poses[4]), pose_error(weighted['transform'], poses[4])
    print(f'box of {n_box}, neighbors {neighbors}: plain {a[0] * 100:.2f} cm / {a[1] * 1e3:.2f} mrad, weighted {b[0] * 100:.2f} cm / '
          f"{b[1] * 1e3:.2f} mrad; {weighted['weight_sum']:.0f} of {weighted['n_corr']} pairs by weight")
    assert plain['status'] == 1 and weighted['status'] == 1
    assert b[0] < a[0] / 3.0 and b[1] < a[1] / 3.0
    assert weighted['n_corr'] > 3000 and weighted['weight_sum'] < weighted['n_corr']


def refine_sequentially(clouds, base, neighbors, robust_scale):
    """trajectory.refine_against_map restated on the restatements (1 m voxels) -> the refined poses."""
    table = MR.Moments(1.0, 3).integrate([clouds[0]], [base[0]])
    out = [base[0]]
    for k in range(1, len(clouds)):
        init = out[k - 1] @ np.linalg.inv(base[k - 1]) @ base[k]
        res = WR.register(table, clouds[k], init, neighbors=neighbors, robust_scale=robust_scale)
        out.append(init if res['status'] == 2 else res['transform'])
        table.integrate([clouds[k]], [out[k]])
    return np.stack(out)


@pytest.mark.parametrize('neighbors', (1, 7))
def test_sequential_refinement_with_a_box_that_moves(neighbors):
    """Eight frames, a box of 800 points that moves 0.3 m from frame to frame, frames 1 .. 7 perturbed by 5 cm / 5 mrad per axis
    (8.74 cm off on average): the plain refinement leaves a larger mean translation error than its input (restatement: 11.8 cm at
    neighbors 1, 34.0 cm at 7), the weighted one less than half the input's (2.0 and 0.9 cm)."""
    clouds, poses = WR.moving_box(np.random.default_rng(2), 800)
    prng = np.random.default_rng(103)
    noisy = np.stack([poses[0]] + [perturb(X, prng, 0.05, 0.005) for X in poses[1:]])

    def mean_error(traj):
        return float(np.mean([pose_error(a, b)[0] for a, b in zip(traj[1:], poses[1:])]))

    before = mean_error(noisy)
    plain, weighted = (mean_error(refine_sequentially(clouds, noisy, neighbors, mu)) for mu in (None, SCALE))
    print(f'neighbors {neighbors}: input {before * 100:.2f} cm, plain {plain * 100:.2f} cm, weighted {weighted * 100:.2f} cm')
    assert plain > before
    assert weighted < 0.5 * before
