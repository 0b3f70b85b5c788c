"""CPU: the map-to-map alignment's declarations and bindings, the `--map-prior-align` options of `python -m rdmnet_amd.trajectory` that
need no GPU, the line format, and the NumPy restatement tests/voxel_align_restatement.py itself: a map against itself does not move,
and two maps of different scans of the street of test_voxel_register, built in frames a known transform apart, find that transform
back from a perturbed start.

The scene (`sessions`) is shared with test_voxel_align_gpu: scans of 4 000 points, session A = scans 0, 2, 4, 6 under their true poses at
1 m voxels (the target), session B = scans 1, 3, 5, 7 under inv(T) pose at 1 m and 0.5 m (the sources), T = 0.3 rad about an axis
near z and a shift of about 3 m.  The two sessions sample the same surfaces with different points, so the alignment ends a centimetre
or two from T: that is the difference between the samplings, not an error of the solver."""
import os
import re

import numpy as np
import pytest

import voxel_align_restatement as AR
import voxel_moments_restatement as MR
import voxel_register_restatement as RR
from rdmnet_amd import _lib, trajectory
from test_voxel_map import write_pairs
from test_voxel_register import perturb, pose_error, street

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'include', 'rdmnet_hip.h')
NEW = ('rdm_voxel_map_align_workspace_bytes', 'rdm_voxel_map_align')
A_SCANS, B_SCANS = (0, 2, 4, 6), (1, 3, 5, 7)
SOURCE_VOXELS = (1.0, 0.5)
# (sigma_t in metres, sigma_r in radians, neighbors) of the perturbed starts, with the seeds 13 and 14 of test_voxel_register_gpu.starts
RECOVERY = ((0.05, 0.005, 1), (0.05, 0.005, 7), (0.3, 0.02, 7))
_cache = {}


def session_transform():
    """T: session A's frame <- session B's."""
    T = RR.apply(np.eye(4), np.array([0.02, -0.03, 0.3, 0.0, 0.0, 0.0]))
    T[:3, 3] = [2.5, -1.5, 0.4]
    return T


def sessions():
    """Computed once, never changed -> (clouds, true poses, T, B's poses in B's frame [8, 4, 4] (all eight scans), the restatement's target,
    {source voxel: the restatement's source})."""
    if 'sessions' not in _cache:
        clouds, poses = street(np.random.default_rng(5), per_scan=4000)
        T = session_transform()
        in_b = np.linalg.inv(T) @ poses
        target = MR.build([clouds[k] for k in A_SCANS], poses[list(A_SCANS)], 1.0, 3)
        sources = {v: MR.build([clouds[k] for k in B_SCANS], in_b[list(B_SCANS)], v, 3) for v in SOURCE_VOXELS}
        _cache['sessions'] = (clouds, poses, T, in_b, target, sources)
    return _cache['sessions']


def starts(seeds=(13, 14), sigma_t=0.05, sigma_r=0.005):
    T = session_transform()
    return np.stack([perturb(T, np.random.default_rng(s), sigma_t, sigma_r) for s in seeds])


def state_of(table, num_scans):
    """What ops.VoxelMap.state would return for the restatement's map (host arrays)."""
    m = table.map
    counters = dict(zip(_lib.VOXEL_MAP_STATS, (len(m.keys), int(m.counts.sum()), m.skipped['skipped_nonfinite'], m.skipped['skipped_range'],
                                               m.skipped['out_of_extent'], 0)))
    return dict(keys=m.keys, counts=m.counts.astype(np.uint32), sums=m.sums, moments=table.sums, voxel=m.voxel, channels=m.channels,
                num_scans=num_scans, counters=counters)


def test_header_declares_the_entry_points_and_bindings_have_them():
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', text), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r'^(?:size_t|int) ' + name + r'\(([^;]*)\);', text, re.M).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in decl.split(',') if a.strip()]), name
    assert 'tests/voxel_align_restatement.py' in text
    assert text.index('voxel map registration') < text.index('voxel map alignment') < text.index('voxel observations:')
    assert _lib.ABI_VERSION == 2 and re.search(r'#define RDM_ABI_VERSION 2\b', text)  # new entry points do not bump it
    # the target comes as register's does: the map's head, the moments block, the voxel
    sig, reg = _lib.SIGNATURES['rdm_voxel_map_align'][1], _lib.SIGNATURES['rdm_voxel_map_register'][1]
    assert sig[:7] == reg[:7]
    assert sig[-8:] == reg[-8:]  # the five outputs, the workspace and the stream
    assert _lib.SIGNATURES['rdm_voxel_map_align_workspace_bytes'] == _lib.SIGNATURES['rdm_voxel_map_register_workspace_bytes']


# ---- the command line --------------------------------------------------------------------------------------------------------

def parse(argv):
    return trajectory.make_parser().parse_args(argv)


def test_align_options_parse_and_need_their_flags(tmp_path):
    from rdmnet_amd import ops
    a = parse(['--features-root', 'x'])
    assert a.map_prior_align is False and a.map_prior_initial is None
    a = parse(['--features-root', 'x', '--map-prior', 'p.npz', '--map-prior-align', '--map-prior-initial', 't.txt'])
    assert a.map_prior_align is True and a.map_prior_initial == 't.txt'
    pairs, root = tmp_path / 'pairs', tmp_path / 'data'
    pairs.mkdir()
    write_pairs(str(pairs), 7, [0, 10])
    folder = root / 'downsampled_xyzi' / '07'
    os.makedirs(folder)
    for f in (0, 10):
        np.save(folder / ('%06d.npy' % f), np.zeros((4, 4), np.float32))
    table = MR.build([np.random.default_rng(0).uniform(-3, 3, (200, 3)).astype(np.float32)], [np.eye(4)], 1.0, 3)
    full_prior, bare_prior = str(tmp_path / 'full.npz'), str(tmp_path / 'bare.npz')
    ops.write_state(full_prior, state_of(table, 1))
    ops.write_state(bare_prior, {k: v for k, v in state_of(table, 1).items() if k != 'moments'})
    lines = []
    base = ['--features-root', str(pairs)]
    full = base + ['--map-scans', str(root), '--out', str(tmp_path / 'o')]

    def refused(argv, message):
        with pytest.raises(trajectory.TrajectoryError, match=message):
            trajectory.run(parse(argv), emit=lines.append)

    for argv in (base + ['--map-prior-align'], full + ['--map-prior-align'], base + ['--map-prior-align', '--map-prior', full_prior],
                 base + ['--map-prior-align', '--map-prior', full_prior, '--map-scans', str(root)],
                 base + ['--map-prior-align', '--map-prior', full_prior, '--out', str(tmp_path / 'o')]):
        refused(argv, '--map-prior-align needs --map-prior, --map-scans and --out')
    good = str(tmp_path / 'start.txt')
    np.savetxt(good, np.eye(4))
    for argv in (base + ['--map-prior-initial', good], full + ['--map-prior-initial', good],
                 full + ['--map-prior', full_prior, '--map-localize', '--map-prior-initial', good]):
        refused(argv, '--map-prior-initial needs --map-prior-align')
    refused(full + ['--map-prior-align', '--map-prior', bare_prior], '--map-prior-align needs a prior with moments')
    missing = str(tmp_path / 'none.txt')
    refused(full + ['--map-prior-align', '--map-prior', full_prior, '--map-prior-initial', missing], re.escape(missing) + ': no such file')
    for name, text in (('short.txt', '1 0 0 0 1 0 0 0 1'), ('words.txt', 'one two three'), ('nan.txt', ' '.join(['nan'] * 12)),
                       ('row.txt', ' '.join(['1'] * 16))):
        path = str(tmp_path / name)
        open(path, 'w').write(text)
        refused(full + ['--map-prior-align', '--map-prior', full_prior, '--map-prior-initial', path], re.escape(path) + ': ')
    # the --map-refine-* options are the alignment's too, with their checks
    refused(full + ['--map-prior-align', '--map-prior', full_prior, '--map-refine-sigma', '0'], '--map-refine-sigma must be > 0')
    refused(full + ['--map-prior-align', '--map-prior', full_prior, '--map-refine-iterations', '-1'], '--map-refine-iterations >= 0')
    refused(full + ['--map-prior-align', '--map-prior', full_prior, '--map-refine-min-scans', '2'], '--map-refine-min-scans needs --map-refine')
    refused(full + ['--map-prior', full_prior], '--map-prior needs --map-clean or --map-localize')  # as before
    assert lines == []  # found before anything is reported
    assert not os.path.exists(tmp_path / 'o')
    with pytest.raises(SystemExit, match='--map-prior-initial needs --map-prior-align'):
        trajectory.main(base + ['--map-prior-initial', good])


def test_read_transform_takes_12_or_16_numbers(tmp_path):
    T = session_transform()
    for rows in (3, 4):
        path = str(tmp_path / f'{rows}.txt')
        np.savetxt(path, T[:rows], fmt='%.17e')
        assert np.array_equal(trajectory.read_transform(path), T)


def test_align_line_format():
    prior = dict(name='5_chained_map_state.npz', voxels=1234, voxel=1.0, scans=4, moments=True)
    stats = dict(status=1, iterations=7, correspondences=6284, cost=1234.5678, matched=1059, voxels=1212, moved_m=0.0691, moved_deg=1.0625)
    assert trajectory.align_line(5, 'chained', prior, stats) == (
        'seq 5 chained aligned to the prior map 5_chained_map_state.npz: 1059 of 1212 voxels matched, 6284 correspondences, 7 iterations, '
        'cost 1234.57, moved 0.069 m / 1.062 deg (converged)')
    assert trajectory.align_line(0, 'optimized', prior, dict(stats, status=0)).endswith('(max_iteration)')


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_a_map_aligned_to_itself_does_not_move():
    """At the identity a voxel's mean maps onto itself bit for bit (1 x + 0 y + 0 z + 0), and it lies in its own voxel: with the own
    cell alone every residual is exactly zero, so g = 0, the update is zero and the pose stays.  With the six neighbours the pairs
    (i, j) and (j, i) have opposite residuals under one M = (Sigma_i + Sigma_j + sigma^2 I)^-1: the translation half of g cancels to
    rounding (the rotation half is sum r x M r, which has no reason to)."""
    _, _, _, _, target, _ = sessions()
    e = AR.evaluate(target, target, np.eye(4), neighbors=1)
    assert e['n_corr'] == e['n_points'] == int((target.map.counts >= 4).sum()) > 1000
    assert not e['g'].any() and e['cost'] == 0.0
    res = AR.align(target, target, np.eye(4), neighbors=1)
    assert res['status'] == 1 and res['iterations'] == 1 and np.array_equal(res['transform'], np.eye(4))
    e7 = AR.evaluate(target, target, np.eye(4), neighbors=7)
    assert e7['n_corr'] > 3 * e['n_corr']
    assert (np.abs(e7['g'][3:]) <= 2.0 ** -52 * e7['n_corr'] * e7['abs_g'][3:]).all()


def test_gates_and_counts():
    _, _, T, _, target, sources = sessions()
    src = sources[0.5]
    for least in (1, 4, 9):
        e = AR.evaluate(target, src, T, source_min_points=least, neighbors=1)
        assert e['n_points'] == int((src.map.counts >= least).sum())
    far = T.copy()
    far[:3, 3] += [1000.0, -2000.0, 50.0]
    res = AR.align(target, src, far)
    assert res['status'] == 2 and res['n_corr'] == 0 and res['iterations'] == 0 and np.array_equal(res['transform'], far)
    assert AR.evaluate(target, src, T, min_points=10 ** 6)['n_corr'] == 0
    out = T.copy()
    out[0, 3] = 2.0 ** 21  # beyond the target's extent at 1 m voxels
    assert AR.evaluate(target, src, out)['n_points'] == 0


@pytest.mark.parametrize('source_voxel', SOURCE_VOXELS)
def test_recovery_of_the_transform_between_two_sessions(source_voxel):
    _, _, T, _, target, sources = sessions()
    for sigma_t, sigma_r, neighbors in RECOVERY:
        for X0 in starts((13, 14), sigma_t, sigma_r):
            res = AR.align(target, sources[source_voxel], X0, neighbors=neighbors)
            before, after = pose_error(X0, T), pose_error(res['transform'], T)
            print(f'source voxel {source_voxel}, neighbors {neighbors}: {before[0] * 100:.2f} cm / {before[1] * 1e3:.2f} mrad -> '
                  f"{after[0] * 100:.2f} cm / {after[1] * 1e3:.2f} mrad, {res['iterations']} updates, status {res['status']}, "
                  f"{res['n_corr']} pairs of {res['n_points']} source voxels")
            assert res['status'] == 1 and res['n_corr'] > 1000
            assert after[0] < before[0] and after[1] < before[1]
