"""CPU: the host side of `python -m rdmnet_amd.prepare` (pair selection, calibration, pose composition, the pair-file
line) against literal restatements of preporcess/generate_kitti_pairs.py, and the argument errors of the new entry
points."""
import ctypes
import os

import numpy as np
import pytest

from rdmnet_amd import _lib, dataset, prepare


def reference_loop(inames, Ts, thres, cap=20000):
    """generate_kitti_pairs.py:118-186 as written (pdist over all frames, the `in inames` tests on a numpy value);
    None where it never ends."""
    pdist = (Ts.reshape(1, -1, 3) - Ts.reshape(-1, 1, 3)) ** 2
    pdist = np.sqrt(pdist.sum(-1))
    more_than_10 = pdist > thres
    curr_time = inames[0]
    pairs, steps = [], 0
    while curr_time in inames:
        steps += 1
        if steps > cap:
            return None
        next_time = np.where(more_than_10[curr_time][curr_time:curr_time + 100])[0]
        if len(next_time) == 0:
            curr_time += 1
        else:
            next_time = next_time[0] + curr_time - 1
        # (an empty array is never `in` the list: the no-frame branch makes no pair)
        if not isinstance(next_time, np.ndarray) and next_time in inames:
            pairs.append((int(curr_time), int(next_time)))
            curr_time = next_time + 1
    return pairs


def track(speeds):
    """Positions along x for per-frame speeds (m/frame), with a small sideways wiggle."""
    x = np.concatenate([[0.0], np.cumsum(speeds)])
    return np.stack([x, 0.3 * np.sin(np.arange(len(x)) / 7.0), 0.01 * np.arange(len(x))], 1)


TRACKS = {
    'steady': (track(np.full(80, 1.1)), None),
    'stop_longer_than_the_window': (track(np.r_[np.full(20, 1.3), np.zeros(150), np.full(40, 1.3)]), None),
    'consecutive_frames_already_far': (track(np.r_[np.full(10, 12.0), np.full(30, 1.0)]), None),
    'ends_inside_the_window': (track(np.full(34, 0.9)), None),
    'last_frame_closes_a_pair': (track(np.full(20, 1.05)), None),
    'gap_ends_the_loop': (track(np.full(60, 1.1)), [20, 21]),
    'gap_inside_a_pair': (track(np.full(60, 1.1)), [4, 5]),
    'gap_at_the_start': (track(np.full(60, 1.1)), [0, 1, 2]),
}


@pytest.mark.parametrize('name', sorted(TRACKS))
def test_pair_frames_matches_the_reference_loop(name):
    Ts, missing = TRACKS[name]
    ids = [i for i in range(len(Ts)) if not missing or i not in missing]
    want = reference_loop(ids, Ts, 10)
    assert want is not None
    got = prepare.pair_frames(ids, Ts, 10)
    assert got == want
    if name == 'consecutive_frames_already_far':
        assert (0, 0) in got  # next == curr
    if name == 'stop_longer_than_the_window':
        assert any(b != e + 1 for (_, e), (b, _) in zip(got, got[1:]))  # the no-frame branch advanced curr one by one
    if name == 'last_frame_closes_a_pair':
        assert got[-1][1] == len(Ts) - 2  # the last frame is the far one that ends the last pair


def test_pair_frames_raises_where_the_reference_never_ends():
    Ts = track(np.full(60, 1.1))
    ids = [i for i in range(60) if i != 9]  # 0 -> the first far frame is 10, so next = 9: not a frame id
    assert reference_loop(ids, Ts, 10) is None
    with pytest.raises(ValueError, match='loops forever'):
        prepare.pair_frames(ids, Ts, 10)
    with pytest.raises(ValueError, match='no pose'):
        prepare.pair_frames([0, 1, 2, 3], Ts[:3], 100)


def rot(ax, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (0, 2), (0, 1)][ax]
    R = np.eye(3)
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


TR = rigid(rot(0, -90) @ rot(2, -90) @ rot(1, 0.3), [-0.004, -0.076, -0.27])


def write_calib(path, Tr, trailing=''):
    with open(path, 'w') as f:
        for k in range(4):
            P = np.zeros((3, 4))
            P[:, :3] = np.eye(3) * (700 + k)
            f.write(f'P{k}: ' + ' '.join(f'{v:.12e}' for v in P.reshape(-1)) + '\n')
        f.write('Tr: ' + ' '.join(f'{v:.12e}' for v in Tr[:3].reshape(-1)) + '\n')
        f.write(trailing)


def test_calib_last_parseable_line_wins_and_M_maps_curr_into_next(tmp_path):
    p = tmp_path / 'calib.txt'
    write_calib(p, TR, trailing='calib_time: 09-Jan-2012 13:57:47\n\nshort: 1 2 3\n')
    velo2cam = prepare.read_velo2cam(str(p))
    assert np.allclose(velo2cam, TR.T, atol=1e-12)  # the reference keeps Tr transposed
    P0 = rigid(rot(1, 3.0), [1.0, 0.2, 5.0])
    P1 = rigid(rot(1, 4.5), [1.4, 0.21, 14.0])
    M = prepare.relative_transform(velo2cam, P0, P1)
    want = np.linalg.inv(TR) @ np.linalg.inv(P1) @ P0 @ TR  # velo(curr) -> cam(curr) -> world -> cam(next) -> velo(next)
    assert np.abs(M - want).max() < 1e-12
    assert np.array_equal(M, (velo2cam @ P0.T @ np.linalg.inv(P1.T) @ np.linalg.inv(velo2cam)).T)
    bad = tmp_path / 'bad.txt'
    bad.write_text('calib_time: 09-Jan-2012\n')
    with pytest.raises(ValueError):
        prepare.read_velo2cam(str(bad))


def test_poses_file_rows(tmp_path):
    P = [rigid(rot(1, 2.0 * k), [0.1 * k, 0.0, 1.1 * k]) for k in range(3)]
    path = tmp_path / '00.txt'
    path.write_text(''.join(' '.join(f'{v:.9e}' for v in T[:3].reshape(-1)) + '\n' for T in P))
    got = prepare.read_poses(str(path))
    assert got.shape == (3, 4, 4) and np.abs(got - np.stack(P)).max() < 1e-9


def test_pair_line_format_and_round_trip(tmp_path):
    T = rigid(rot(2, 1.25) @ rot(0, -0.2), [-0.0123456789, 11.5, -0.5])
    line = prepare.format_pair_line(12, 20, T)
    assert line.endswith(' \n') and line.startswith('12 20 ')
    assert line == '12 20 ' + ' '.join(f'{v:.6f}' for v in T[:3].reshape(-1)) + ' \n'
    (tmp_path / '08').write_text(line + prepare.format_pair_line(21, 29, np.eye(4)))
    items = dataset.load_kitti_gt_txt(str(tmp_path), 8)
    assert [(d['frame1'], d['frame0']) for d in items] == [(12, 20), (21, 29)]  # frame1 = anc = curr (the ICP source)
    assert np.abs(items[0]['transform'] - T).max() <= 5e-7 and np.array_equal(items[1]['transform'], np.eye(4))


@pytest.mark.parametrize('argv', [
    [],
    ['unknown', '--dataset-root', '.'],
    ['pairs'],
    ['pairs', '--dataset-root', '.', '--distance', '0'],
    ['pairs', '--dataset-root', '.', '--distance', '-0.5'],
    ['pairs', '--dataset-root', '.', '--max-iteration', '-1'],
    ['pairs', '--dataset-root', '.', '--thres', '-3'],
    ['pairs', '--dataset-root', '.', '--sequences', '-1'],
    ['downsample', '--dataset-root', '/nonexistent/kitti'],
])
def test_cli_argument_errors(argv):
    with pytest.raises(SystemExit) as e:
        prepare.main(argv)
    assert e.value.code == 2


def test_missing_scans_are_an_error(tmp_path):
    with pytest.raises(FileNotFoundError):
        prepare.frame_ids(str(tmp_path), 8)


def test_icp_entry_points_reject_bad_arguments_before_touching_the_device():
    L = _lib.lib()
    out = (ctypes.c_double * 32)()
    st = (ctypes.c_int32 * 2)()
    p = ctypes.addressof(out)
    for r in (0.0, -0.5):
        assert L.rdm_icp_point_to_point(0, 0, 3, 0, 0, 3, r, None, 30, 1e-6, 1e-6, p, p, ctypes.addressof(st), None, None, 0,
                                        None) == -1
        assert b'max_correspondence_distance' in L.rdm_last_error()
        assert L.rdm_icp_correspondences(0, 0, 0, 0, 3, r, ctypes.addressof(st), p, None, 0, None) == -1
        assert b'max_correspondence_distance' in L.rdm_last_error()
    assert L.rdm_icp_point_to_point(0, 0, 3, 0, 0, 3, 0.5, None, -1, 1e-6, 1e-6, p, p, ctypes.addressof(st), None, None, 0,
                                    None) == -1
    assert L.rdm_icp_point_to_point(0, 0, 2, 0, 0, 3, 0.5, None, 30, 1e-6, 1e-6, p, p, ctypes.addressof(st), None, None, 0,
                                    None) == -1  # row stride below 3
    assert L.rdm_icp_point_to_point(0, 10, 3, 0, 0, 3, 0.5, None, 30, 1e-6, 1e-6, p, p, ctypes.addressof(st), None, None, 0,
                                    None) == -1  # null source with points
    assert L.rdm_icp_point_to_point(0, 0, 3, 0, 0, 3, 0.5, None, 30, 1e-6, 1e-6, None, p, ctypes.addressof(st), None, None, 0,
                                    None) == -1  # null output


def test_icp_restatement_recovers_a_small_motion():
    """The float64 restatement the GPU tests compare against, on its own: a noise-free subset moved by a small rigid
    motion comes back to the inverse motion."""
    import icp_restatement as ir
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-10, 10, (3000, 3)).astype(np.float32)
    src = tgt[::2].astype(np.float64)
    G = rigid(rot(2, 0.3) @ rot(0, 0.1), [0.1, -0.05, 0.02])
    moved = ir.apply(G, src).astype(np.float32)
    T, fit, rmse, n, it = ir.icp(moved, tgt, 0.5, max_iteration=100)
    assert np.abs(T @ G - np.eye(4)).max() < 1e-5 and fit > 0.99 and 0 < it < 100
