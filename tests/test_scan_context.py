"""CPU: the float64 restatement of Scan Context (tests/scan_context_restatement.py) on its own fixtures, the new C-ABI symbols, and
the host sides of `python -m rdmnet_amd.prepare loops` and `python -m rdmnet_amd.infer --pair-lists`.

The conditions the GPU test (tests/test_scan_context_gpu.py) relies on are asserted here, on the CPU: on the bundled scans few bins
have a point so close to a bin edge that another rounding of atan2 or of the radius could change the bin's VALUE (measured: 0, 3
and 2 of 1 200 bins; bound 5 %; the bins merely touched by such a point, whatever holds their maximum, number 15, 25 and 15), and on the seeded random descriptors few pairs have two shifts within 1e-4 of each other
(measured 0.41 %; bound 1 %)."""
import os
import re

import numpy as np
import pytest

import scan_context_restatement as SC
from rdmnet_amd import _lib, dataset, prepare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROTATIONS = ((91.0, 15), (33.0, 5), (200.0, 33), (-47.0, 52))


def test_rotated_copies_recover_their_shift(scans):
    s0 = scans['s000000']
    D0 = SC.descriptor(s0)
    for deg, want in ROTATIONS:
        d, shift, margin = SC.distance(SC.descriptor(SC.rotate_z(s0, deg)), D0)
        print(deg, d, shift, margin)
        assert shift == want
    d, shift, margin = SC.distance(SC.descriptor(SC.rotate_z(s0, 91.0)), D0)
    assert abs(d - 0.0442) < 1e-4 and abs(d + margin - 0.205) < 1e-3
    # the other two bundled scans are 4 and 7 frames away: similar, but above the default threshold
    assert abs(SC.distance(SC.descriptor(scans['s000007']), D0)[0] - 0.309) < 1e-3


def test_self_distance_and_shift_symmetry(scans):
    Ds = [SC.descriptor(scans[k]) for k in ('s000000', 's000004', 's000007')]
    for D in Ds:
        d, shift, _ = SC.distance(D, D)
        assert d == 0.0 and shift == 0
    S = Ds[0].shape[1]
    for Q, C in ((SC.descriptor(SC.rotate_z(scans['s000000'], 91.0)), Ds[0]), (Ds[1], Ds[0]), (Ds[2], Ds[1])):
        a, b = SC.shift_distances(Q, C), SC.shift_distances(C, Q)
        assert np.allclose(a, b[(S - np.arange(S)) % S], rtol=0, atol=1e-14)  # d_n(Q, C) = d_{(S - n) mod S}(C, Q)
        assert SC.distance(C, Q)[1] == (S - SC.distance(Q, C)[1]) % S


def test_values_may_be_negative_and_empty_bins_are_zero(scans):
    D = SC.descriptor(scans['s000000'])
    assert D.dtype == np.float32 and D.shape == (20, 60)
    assert -0.8 < D.min() < -0.7  # heights below the sensor's assumed 2 m: the maximum must order negative floats
    assert (D == 0).mean() > 0.3
    pts = np.array([[1.0, 0.1, -5.0], [1.0, 0.1, -7.0], [np.nan, 1, 1], [0, 0, 9], [80.0, 0.0, 1.0], [80.001, 0.0, 5.0]], np.float32)
    E = SC.descriptor(pts)
    assert E[0, 0] == np.float32(-3.0) and E[19, 0] == np.float32(3.0) and np.count_nonzero(E) == 2
    assert not SC.descriptor(np.zeros((0, 3), np.float32)).any()


def test_few_bins_of_the_bundled_scans_depend_on_rounding(scans):
    for k in ('s000000', 's000004', 's000007'):
        D, lo, hi = SC.descriptor_interval(scans[k])
        assert (lo <= D).all() and (D <= hi).all()
        loose = int((lo != hi).sum())
        print(k, loose, 'of', D.size, 'bins with lo != hi')
        assert loose <= 0.05 * D.size
    # a point 1e-6 rad from a sector edge and one on a ring edge: their bins and the neighbours open up, the rest stay exact
    w = 2 * np.pi / 60
    pts = np.array([[10 * np.cos(3 * w + 1e-6), 10 * np.sin(3 * w + 1e-6), 1.0], [4.8, 6.4, -3.0], [30.0, -20.0, 0.5]], np.float32)
    D, lo, hi = SC.descriptor_interval(pts)
    assert (lo <= D).all() and (D <= hi).all() and (lo != hi).sum() == 4
    assert lo[2, 2] == 0 and hi[2, 2] == 3 and lo[2, 3] == 0 and hi[2, 3] == 3
    assert lo[1, 8] == -1 and hi[1, 8] == 0 and lo[2, 8] == -1 and hi[2, 8] == 0


def test_random_fixture_has_clear_shifts():
    Q, C = SC.random_fixture()
    assert Q.shape == (37, 20, 60) and C.shape == (53, 20, 60)
    assert 0.5 < (Q == 0).mean() < 0.6 and (np.abs(Q).sum(1) == 0).any()  # half the bins and some whole columns empty
    d, s, m = SC.distance_matrix(Q, C)
    frac = float((m < 1e-4).mean())
    print('pairs with a shift margin below 1e-4:', frac)
    assert frac <= 0.01


def test_search_windows_and_ties():
    d = np.array([[0.5, 0.2, 0.2, 0.9], [0.1, 0.3, 0.05, 0.0], [0.7, 0.7, 0.7, 0.7]])
    idx, best, gap = SC.search(d, exclude_recent=-1)
    assert idx.tolist() == [1, 3, 0] and best.tolist() == [0.2, 0.0, 0.7] and gap[0] == 0.0
    idx, best, _ = SC.search(d, exclude_recent=1)  # candidate j for query i iff i - j >= 1
    assert idx.tolist() == [-1, 0, 0] and np.isinf(best[0]) and best[1] == 0.1
    idx, _, _ = SC.search(d, q_base=10, c_base=8, exclude_recent=3)  # (10 + i) - (8 + j) >= 3
    assert idx.tolist() == [-1, 0, 0]
    assert SC.search(d, exclude_recent=100)[0].tolist() == [-1, -1, -1]


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'rdmnet_hip.h')).read()
    L = _lib.lib()
    for n in ('rdm_scan_context', 'rdm_scan_context_workspace_bytes', 'rdm_scan_context_distance',
              'rdm_scan_context_distance_workspace_bytes'):
        assert re.search(r'\b' + n + r'\s*\(', text) and hasattr(L, n) and n in _lib.SIGNATURES
    assert int(re.search(r'#define RDM_SCAN_CONTEXT_MAX_DIM (\d+)', text).group(1)) == _lib.SCAN_CONTEXT_MAX_DIM
    assert int(re.search(r'#define RDM_SCAN_CONTEXT_LD (\d+)', text).group(1)) == _lib.SCAN_CONTEXT_LD
    assert L.rdm_abi_version() == 2
    # host-only: the workspaces grow with their arguments; parameters outside 1 ... 64 have none
    sizes = [L.rdm_scan_context_workspace_bytes(n, 20, 60) for n in (1, 8, 64, 4541)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < (1 << 30)
    assert L.rdm_scan_context_workspace_bytes(64, 20, 60) < L.rdm_scan_context_workspace_bytes(64, 40, 64)
    sizes = [L.rdm_scan_context_distance_workspace_bytes(n, n, 20, 60) for n in (1, 37, 4541, 100000)]
    assert all(0 < a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < (1 << 31)
    assert L.rdm_scan_context_distance_workspace_bytes(37, 53, 20, 60) < L.rdm_scan_context_distance_workspace_bytes(37, 5300, 20, 60)
    for r, s in ((0, 60), (20, 0), (65, 60), (20, 65), (-1, 60)):
        assert L.rdm_scan_context_workspace_bytes(8, r, s) == 0
        assert L.rdm_scan_context_distance_workspace_bytes(8, 8, r, s) == 0
    assert L.rdm_scan_context_workspace_bytes(-1, 20, 60) == 0 and L.rdm_scan_context_distance_workspace_bytes(8, -1, 20, 60) == 0
    # rejected parameters are an error code before anything is launched or read (null pointers here)
    assert L.rdm_scan_context(0, 3, 0, 0, 1, 65, 60, 80.0, 2.0, 0, 0, 0, 0, 0, 0) == -1
    assert b'n_rings' in L.rdm_last_error()
    assert L.rdm_scan_context_distance(0, 1, 0, 1, 20, 0, 0, 0, 50, 0, 0, 0, 0, 0, 0, 0, 0) == -1


def test_ops_reject_bad_arguments_by_name():
    import torch
    from rdmnet_amd import ops
    with pytest.raises(ValueError, match=r'clouds\[0\]'):
        ops.scan_context([torch.zeros(4, 3)])  # not on the GPU
    with pytest.raises(ValueError, match='n_rings'):
        ops.scan_context([torch.zeros(4, 3)], n_rings=65)
    with pytest.raises(ValueError, match='q_desc'):
        ops.scan_context_distance(torch.zeros(2, 20, 60), torch.zeros(2, 20, 60))
    with pytest.raises(ValueError, match='q_desc'):
        ops.detect_loops(torch.zeros(2, 20, 60, dtype=torch.float64))


def test_prepare_loops_parser_and_line_formats():
    a = prepare._parser().parse_args(['loops', '--dataset-root', 'R'])
    assert (a.command, a.threshold, a.exclude_recent, a.raw, a.batch, a.sequences) == ('loops', 0.13, 50, False, 64, list(range(11)))
    b = prepare._parser().parse_args(['loops', '--dataset-root', 'R', '--sequences', '0', '8', '--threshold', '0.2', '--exclude-recent',
                                      '-1', '--raw', '--batch', '16'])
    assert (b.sequences, b.threshold, b.exclude_recent, b.raw, b.batch) == ([0, 8], 0.2, -1, True, 16)
    assert prepare.format_score_line(3, 0, 0.0441723, 15, 90.0) == '3 0 0.044172 15 90.0\n'
    line = prepare.format_pair_line(3, 0, prepare.yaw_transform(15))
    assert line == '3 0 0.000000 1.000000 0.000000 0.000000 -1.000000 0.000000 0.000000 0.000000 0.000000 0.000000 1.000000 0.000000 \n'


def test_loop_list_reads_back_as_src_query_ref_candidate(tmp_path, scans):
    """The written line makes the query the src scan and the candidate the ref scan of the dataset, and the yaw-only pose maps the
    query onto the candidate: for a query that is the candidate turned by 90 degrees every point lands within half a sector."""
    cand = scans['s000000']
    query = SC.rotate_z(cand, 90.0)
    d, shift, _ = SC.distance(SC.descriptor(query), SC.descriptor(cand))
    assert shift == 15
    T = prepare.yaw_transform(shift)
    os.makedirs(tmp_path / 'loops')
    (tmp_path / 'loops' / '00').write_text(prepare.format_pair_line(3, 0, T))
    meta = dataset.load_kitti_gt_txt(str(tmp_path / 'loops'), 0)
    assert len(meta) == 1 and (meta[0]['frame1'], meta[0]['frame0']) == (3, 0)  # frame1 = src = query, frame0 = ref = candidate
    moved = query[:, :3].astype(np.float64) @ meta[0]['transform'][:3, :3].T + meta[0]['transform'][:3, 3]
    far = np.linalg.norm(cand[:, :2], axis=1) > 1.0
    ang = np.arctan2(moved[far, 1], moved[far, 0]) - np.arctan2(cand[far, 1].astype(np.float64), cand[far, 0].astype(np.float64))
    ang = np.abs((ang + np.pi) % (2 * np.pi) - np.pi)
    assert np.rad2deg(ang.max()) < 3.0 and np.abs(moved - cand).max() < 1e-4


def test_ground_truth_branch_is_relative_transform(tmp_path):
    rng = np.random.default_rng(5)
    os.makedirs(tmp_path / 'poses')
    os.makedirs(tmp_path / 'calib' / 'sequences' / '03')
    assert prepare.loop_ground_truth(str(tmp_path), 3) is None
    assert np.array_equal(prepare.loop_transform(None, 70, 2, 7), prepare.yaw_transform(7))
    poses = rng.normal(size=(80, 12))
    np.savetxt(tmp_path / 'poses' / '03.txt', poses)
    tr = rng.normal(size=12)
    (tmp_path / 'calib' / 'sequences' / '03' / 'calib.txt').write_text('P0: 1 0 0 0 0 1 0 0 0 0 1 0\nTr: ' + ' '.join(repr(float(v)) for v in tr) + '\n')
    gt = prepare.loop_ground_truth(str(tmp_path), 3)
    velo2cam, P = prepare.read_velo2cam(str(tmp_path / 'calib' / 'sequences' / '03' / 'calib.txt')), prepare.read_poses(str(tmp_path / 'poses' / '03.txt'))
    assert np.array_equal(gt[0], velo2cam) and np.array_equal(gt[1], P)
    assert np.array_equal(prepare.loop_transform(gt, 70, 2, 7), prepare.relative_transform(velo2cam, P[70], P[2]))
    with pytest.raises(ValueError):
        prepare.loop_transform(gt, 80, 2, 7)


def test_scan_list_reads_either_tree(tmp_path):
    os.makedirs(tmp_path / 'downsampled_xyzi' / '00')
    os.makedirs(tmp_path / 'sequences' / '00' / 'velodyne')
    pts = np.arange(20, dtype=np.float32).reshape(5, 4)
    for f in (2, 0, 1):
        np.save(tmp_path / 'downsampled_xyzi' / '00' / ('%06d.npy' % f), pts + f)
        (pts - f).tofile(tmp_path / 'sequences' / '00' / 'velodyne' / ('%06d.bin' % f))
    for raw, sign in ((False, 1), (True, -1)):
        lst = prepare.scan_list(str(tmp_path), 0, raw)
        assert [f for f, _ in lst] == [0, 1, 2]
        assert np.array_equal(prepare.load_scan_xyz(lst[2][1]), (pts + sign * 2)[:, :3])
    with pytest.raises(FileNotFoundError):
        prepare.scan_list(str(tmp_path), 1)


def test_infer_pair_lists_parse_and_metadata(tmp_path):
    from rdmnet_amd import infer
    a = infer.make_parser().parse_args(['--dataset-root', 'R', '--pair-lists', 'loops', '--sequences', '0', '5', '--information'])
    assert (a.pair_lists, a.sequences, a.information, a.subset) == ('loops', [0, 5], True, 'test')
    d = infer.make_parser().parse_args(['--dataset-root', 'R'])
    assert d.pair_lists is None and d.sequences is None
    os.makedirs(tmp_path / 'loops')
    os.makedirs(tmp_path / 'icp10')
    (tmp_path / 'loops' / '00').write_text(prepare.format_pair_line(120, 3, prepare.yaw_transform(15)) +
                                           prepare.format_pair_line(130, 9, prepare.yaw_transform(59)))
    (tmp_path / 'loops' / '05').write_text(prepare.format_pair_line(400, 7, np.eye(4)))
    (tmp_path / 'loops' / '00.scores').write_text(prepare.format_score_line(120, 3, 0.05, 15, 90.0))
    (tmp_path / 'icp10' / '00').write_text(prepare.format_pair_line(0, 11, np.eye(4)))
    meta, seqs = infer.pair_list_metadata(str(tmp_path), 'loops')
    assert seqs == [0, 5] and [(m['seq_id'], m['frame1'], m['frame0']) for m in meta] == [(0, 120, 3), (0, 130, 9), (5, 400, 7)]
    assert np.allclose(meta[1]['transform'], prepare.yaw_transform(59), atol=1e-6)
    meta, seqs = infer.pair_list_metadata(str(tmp_path), 'loops', [5])
    assert seqs == [5] and len(meta) == 1
    data = dataset.OdometryKittiPairDataset(str(tmp_path), 'test', metadata=meta)
    assert len(data) == 1 and data.metadata[0]['frame1'] == 400
    with pytest.raises(FileNotFoundError):
        infer.pair_list_metadata(str(tmp_path), 'nothing')
