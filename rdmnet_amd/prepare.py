"""Derived KITTI trees from raw data, the two trees `dataset.OdometryKittiPairDataset` reads:

  python -m rdmnet_amd.prepare downsample --dataset-root R [--sequences 0 ... 10]
      R/sequences/%02d/velodyne/*.bin (f32 [N, 4]) -> R/downsampled_xyzi/%02d/<frame>.npy (f32 [M, 4]): centroid voxel
      down-sampling at 0.3 m of xyz + intensity on the GPU (ops.voxel_downsample), as preporcess/downsample_pcd_kitti.py
      does with Open3D.
  python -m rdmnet_amd.prepare pairs --dataset-root R [--sequences 8 9 10] [--thres 10] [--max-iteration 5000]
                                     [--distance 0.5]
      R/poses/%02d.txt + R/calib/sequences/%02d/calib.txt + the raw scans -> R/icp{thres}/%02d: the pair lists with
      ICP-refined poses, restating preporcess/generate_kitti_pairs.py:95-195 with the GPU ICP (ops.icp_point_to_point).

  python -m rdmnet_amd.prepare overlap --dataset-root R [--distance 10] [--radius 0.6]
      R/icp{distance}/%02d + R/downsampled_xyzi -> R/overlap{distance}/%02d, one line per pair of the list:
      `frame0 frame1 overlap_ref overlap_src num_corr` -- compute_overlap both ways and the number of get_correspondences rows at
      `radius` (geotransformer/utils/registration.py:191-216) on the GPU (ops.pair_overlap: one count pass, no list), the
      number the reference's loop-closure protocol selects pairs by (experiments/test_batchoffline.py:246).

  python -m rdmnet_amd.prepare loops --dataset-root R [--sequences 0 ... 10] [--threshold 0.13] [--exclude-recent 50] [--raw]
                                     [--batch 64]
      R/downsampled_xyzi/%02d/*.npy (the tree `infer` reads; --raw: R/sequences/%02d/velodyne/*.bin) -> R/loops/%02d and
      R/loops/%02d.scores: loop-closure detection.  One Scan Context descriptor per scan (ops.scan_context, in batches), every scan
      against every scan at least --exclude-recent frames older under all column shifts on the GPU (ops.detect_loops: exhaustive,
      no prefilter); a loop is accepted below --threshold.  R/loops/%02d has the format of icp10, `query candidate` + the pose
      that maps the query scan into the candidate's frame, so `infer --pair-lists loops` reads it (src = query, ref = candidate):
      the ground-truth pose when R/poses/%02d.txt and the calib file exist, else the yaw-only guess Rz(-shift 360 / 60 deg).
      R/loops/%02d.scores: `query candidate distance shift yaw_deg` per loop.  Not in the reference.

Stated deviations from the reference's pair script:
  * the pair file is written fresh; the reference appends to it (its `open(..., 'a')`), so a rerun doubles it;
  * the odometry pose M is handed to the ICP as its `init` instead of being applied to the scan on the host first: the
    same algorithm, only the rounding of the first transform differs (the file holds reg.transformation @ M, the
    composition the reference's issue.md explains);
  * where the reference would loop forever (the frame before the first far one is not a frame id), this raises.
"""
import argparse
import glob
import os
import os.path as osp
import queue
import threading

import numpy as np

DOWNSAMPLE_VOXEL = 0.3
WINDOW = 100  # frames looked ahead for the next pair (generate_kitti_pairs.py:131)


def read_poses(path):
    """R/poses/%02d.txt -> float64 [F, 4, 4] (camera-frame poses, T_w_cam0), one row per frame."""
    rows = np.genfromtxt(path).reshape(-1, 12)
    pos = np.zeros((rows.shape[0], 4, 4))
    pos[:, :3, :] = rows.reshape(-1, 3, 4)
    pos[:, 3, 3] = 1.0
    return pos


def read_velo2cam(path):
    """calib.txt -> the reference's `velo2cam` (get_velo2cam): the last line whose value parses as 12 floats (Tr in a
    KITTI odometry calib.txt) as a 4x4, TRANSPOSED, as the reference keeps it."""
    calib = None
    with open(path) as f:
        for line in f:
            if ':' not in line:
                continue
            try:
                v = np.array([float(x) for x in line.split(':', 1)[1].split()])
            except ValueError:
                continue
            if v.size == 12:
                calib = v
    if calib is None:
        raise ValueError(f'{path}: no line with 12 values')
    return np.vstack([calib.reshape(3, 4), [0, 0, 0, 1]]).T


def relative_transform(velo2cam, pose0, pose1):
    """generate_kitti_pairs.py:151-152: M maps scan `curr` (pose0) into the velodyne frame of scan `next` (pose1)."""
    return (velo2cam @ pose0.T @ np.linalg.inv(pose1.T) @ np.linalg.inv(velo2cam)).T


def pair_frames(frame_ids, translations, thres, window=WINDOW):
    """The pairing loop of generate_kitti_pairs.py:124-186 -> [(curr, next)].  Frame ids index the rows of
    `translations` directly.  From curr (the first id): the frames curr ... curr+window-1 farther than `thres` from curr;
    none -> curr + 1; else next = (the first of them) - 1 is a pair if it is a frame id, and curr = next + 1.  The loop
    ends when curr is not a frame id."""
    ids = sorted(int(i) for i in frame_ids)
    have = set(ids)
    T = np.asarray(translations, dtype=np.float64)
    pairs = []
    curr = ids[0] if ids else None
    while curr in have:
        if curr >= T.shape[0]:
            raise ValueError(f'frame {curr} has no pose (the pose file has {T.shape[0]} rows)')
        dist = np.sqrt(((T[curr:curr + window] - T[curr]) ** 2).sum(-1))  # = the reference's pdist[curr][curr:curr+window]
        far = np.where(dist > thres)[0]
        if len(far) == 0:
            curr += 1
            continue
        nxt = int(far[0]) + curr - 1
        if nxt not in have:
            raise ValueError(f'frame {nxt} (before the first frame farther than {thres} m from {curr}) is missing: the '
                             'reference loops forever here')
        pairs.append((curr, nxt))
        curr = nxt + 1
    return pairs


def format_pair_line(curr, nxt, transform):
    """One line of R/icp{thres}/%02d: `curr next` and the first three rows of the pose, '%.6f ' each (a trailing blank
    before the newline, as the reference writes it)."""
    v = np.asarray(transform, dtype=np.float64).reshape(-1)[:12]
    return f'{curr} {nxt} ' + ''.join(f'{x:.6f} ' for x in v) + '\n'


def _velodyne(root, seq):
    return osp.join(root, 'sequences', '%02d' % seq, 'velodyne')


def frame_ids(root, seq):
    files = glob.glob(osp.join(_velodyne(root, seq), '*.bin'))
    if not files:
        raise FileNotFoundError(f'no scans under {_velodyne(root, seq)}')
    return sorted(int(osp.basename(f)[:-4]) for f in files)


def read_scan(root, seq, frame):
    return np.fromfile(osp.join(_velodyne(root, seq), '%06d.bin' % frame), dtype=np.float32).reshape(-1, 4)


def _read_ahead(load, keys, depth=2):
    """Yields (key, load(key)) in order; a background thread reads up to `depth` items ahead."""
    q = queue.Queue(maxsize=depth)
    stop = threading.Event()

    def work():
        for k in keys:
            try:
                item = (k, load(k), None)
            except Exception as e:  # surfaced in the consumer
                item = (k, None, e)
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    break
                except queue.Full:
                    continue
            if stop.is_set() or item[2] is not None:
                return

    t = threading.Thread(target=work, daemon=True)
    t.start()
    try:
        for _ in keys:
            k, v, err = q.get()
            if err is not None:
                raise err
            yield k, v
    finally:
        stop.set()


def downsample_sequence(root, seq, voxel=DOWNSAMPLE_VOXEL, log=print):
    """R/sequences/%02d/velodyne/*.bin -> R/downsampled_xyzi/%02d/<frame>.npy (f32 [M, 4])."""
    import torch
    from . import ops
    out_dir = osp.join(root, 'downsampled_xyzi', '%02d' % seq)
    os.makedirs(out_dir, exist_ok=True)
    ids = frame_ids(root, seq)
    for frame, pts in _read_ahead(lambda f: read_scan(root, seq, f), ids):
        got = ops.voxel_downsample(torch.from_numpy(pts).cuda(), voxel).cpu().numpy()
        np.save(osp.join(out_dir, '%06d.npy' % frame), got)
    log(f'sequence {seq:02d}: {len(ids)} scans down-sampled into {out_dir}')
    return len(ids)


class _RawPairs:
    """Items for dataset.PairStager: ref_points = scan `next` (the ICP target), src_points = scan `curr` (the source)."""

    def __init__(self, root, seq, pairs):
        self.root, self.seq, self.pairs = root, seq, pairs

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        curr, nxt = self.pairs[i]
        return {'curr': curr, 'next': nxt, 'ref_points': read_scan(self.root, self.seq, nxt)[:, :3],
                'src_points': read_scan(self.root, self.seq, curr)[:, :3]}


def generate_pairs(root, seq, thres=10, max_iteration=5000, distance=0.5, log=print):
    """R/icp{thres}/%02d for one sequence (generate_kitti_pairs.py:95-195) -> [(curr, next, pose f64 [4, 4])]."""
    from . import ops
    from .dataset import PairStager
    ids = frame_ids(root, seq)
    poses = read_poses(osp.join(root, 'poses', '%02d.txt' % seq))
    velo2cam = read_velo2cam(osp.join(root, 'calib', 'sequences', '%02d' % seq, 'calib.txt'))
    pairs = pair_frames(ids, poses[:, :3, 3], thres)
    out_dir = osp.join(root, 'icp%d' % thres)
    os.makedirs(out_dir, exist_ok=True)
    out = []
    with open(osp.join(out_dir, '%02d' % seq), 'w') as f:
        for item, target, source in PairStager(_RawPairs(root, seq, pairs)):
            curr, nxt = item['curr'], item['next']
            M = relative_transform(velo2cam, poses[curr], poses[nxt])
            reg = ops.icp_point_to_point(source, target, distance, init=M, max_iteration=max_iteration)
            f.write(format_pair_line(curr, nxt, reg.transformation))
            f.flush()
            out.append((curr, nxt, reg.transformation))
    log(f'sequence {seq:02d}: {len(out)} pairs written to {osp.join(out_dir, "%02d" % seq)}')
    return out


class _ListedPairs:
    """Items for dataset.PairStager: the two down-sampled scans of a pair of an icp{distance} list (frame0 = ref, frame1 = src)."""

    def __init__(self, root, metadata):
        self.root, self.metadata = root, metadata

    def __len__(self):
        return len(self.metadata)

    def _scan(self, seq, frame):
        return np.load(osp.join(self.root, 'downsampled_xyzi', '%02d' % seq, '%06d.npy' % frame))[:, :3].astype(np.float32)

    def __getitem__(self, i):
        meta = self.metadata[i]
        return dict(meta, ref_points=self._scan(meta['seq_id'], meta['frame0']), src_points=self._scan(meta['seq_id'], meta['frame1']))


def format_overlap_line(frame0, frame1, overlap_ref, overlap_src, num_corr):
    return f'{frame0} {frame1} {overlap_ref:.6f} {overlap_src:.6f} {num_corr}\n'


def listed_sequences(root, distance):
    """The sequences that have a pair list under R/icp{distance}."""
    files = glob.glob(osp.join(root, 'icp%d' % distance, '[0-9][0-9]'))
    if not files:
        raise FileNotFoundError(f'no pair lists under {osp.join(root, "icp%d" % distance)}')
    return sorted(int(osp.basename(f)) for f in files)


def overlap_sequence(root, seq, distance=10, radius=0.6, workers=4, log=print):
    """R/overlap{distance}/%02d for one sequence -> [(frame0, frame1, overlap_ref, overlap_src, num_corr)].  The scans are read on
    `workers` (at most 16) host threads while the previous pair is on the GPU (dataset.PairStager)."""
    from . import ops
    from .dataset import PairStager, load_kitti_gt_txt
    metadata = load_kitti_gt_txt(osp.join(root, 'icp%d' % distance), seq)
    out_dir = osp.join(root, 'overlap%d' % distance)
    os.makedirs(out_dir, exist_ok=True)
    out = []
    with open(osp.join(out_dir, '%02d' % seq), 'w') as f:
        for item, ref, src in PairStager(_ListedPairs(root, metadata), workers=max(1, min(int(workers), 16))):
            o_ref, o_src, num = ops.pair_overlap(ref, src, item['transform'], radius)
            out.append((item['frame0'], item['frame1'], o_ref, o_src, num))
            f.write(format_overlap_line(*out[-1]))
    log(f'sequence {seq:02d}: {len(out)} pairs written to {osp.join(out_dir, "%02d" % seq)}')
    return out


LOOP_DEFAULTS = dict(threshold=0.13, exclude_recent=50, batch=64)
LOOP_SECTORS = 60  # ops.scan_context's default n_sectors: one column shift is 6 degrees


def scan_list(root, seq, raw=False):
    """[(frame, path)] of a sequence in frame order: R/downsampled_xyzi/%02d/*.npy, or with `raw` R/sequences/%02d/velodyne/*.bin."""
    folder = _velodyne(root, seq) if raw else osp.join(root, 'downsampled_xyzi', '%02d' % seq)
    ext = '.bin' if raw else '.npy'
    files = glob.glob(osp.join(folder, '*' + ext))
    if not files:
        raise FileNotFoundError(f'no scans under {folder}')
    return sorted((int(osp.basename(f)[:-len(ext)]), f) for f in files)


def load_scan(path):
    """One scan of either tree with all its columns -> f32 [N, 4] (xyz + intensity; a .npy may hold other widths)."""
    pts = np.fromfile(path, dtype=np.float32).reshape(-1, 4) if path.endswith('.bin') else np.load(path)
    return np.ascontiguousarray(pts, dtype=np.float32)


def load_scan_xyz(path):
    """One scan of either tree -> f32 [N, 3]."""
    pts = np.fromfile(path, dtype=np.float32).reshape(-1, 4) if path.endswith('.bin') else np.load(path)
    return np.ascontiguousarray(pts[:, :3], dtype=np.float32)


def scan_path(root, seq, frame, raw=False):
    """The file of one frame: R/downsampled_xyzi/%02d/%06d.npy, or with `raw` R/sequences/%02d/velodyne/%06d.bin."""
    if raw:
        return osp.join(_velodyne(root, seq), '%06d.bin' % frame)
    return osp.join(root, 'downsampled_xyzi', '%02d' % seq, '%06d.npy' % frame)


def yaw_transform(shift, n_sectors=LOOP_SECTORS):
    """The yaw-only pose guess of a loop: the query scan is the candidate turned by +shift sectors about z, so Rz(-shift 360 /
    n_sectors degrees) maps the query into the candidate's frame."""
    a = -2.0 * np.pi * shift / n_sectors
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return T


def loop_ground_truth(root, seq):
    """(velo2cam, poses) when R/poses/%02d.txt and R/calib/sequences/%02d/calib.txt exist, else None."""
    poses, calib = osp.join(root, 'poses', '%02d.txt' % seq), osp.join(root, 'calib', 'sequences', '%02d' % seq, 'calib.txt')
    if not (osp.isfile(poses) and osp.isfile(calib)):
        return None
    return read_velo2cam(calib), read_poses(poses)


def loop_transform(gt, query, candidate, shift, n_sectors=LOOP_SECTORS):
    """The pose written for a loop (frame ids): relative_transform of the ground truth (query -> candidate), else yaw_transform."""
    if gt is None:
        return yaw_transform(shift, n_sectors)
    velo2cam, poses = gt
    if max(query, candidate) >= poses.shape[0]:
        raise ValueError(f'frame {max(query, candidate)} has no pose (the pose file has {poses.shape[0]} rows)')
    return relative_transform(velo2cam, poses[query], poses[candidate])


def format_score_line(query, candidate, distance, shift, yaw_deg):
    return f'{query} {candidate} {distance:.6f} {shift} {yaw_deg:.1f}\n'


def sequence_descriptors(root, seq, raw=False, batch=LOOP_DEFAULTS['batch']):
    """-> (frame ids, descriptors float32 CUDA [F, 20, 60]): the scans are read `batch` at a time on a background thread while the
    previous batch is on the GPU; a batch is one host-to-device copy and one ops.scan_context call."""
    import torch
    from . import ops
    scans = scan_list(root, seq, raw)
    batches = [tuple(scans[i:i + batch]) for i in range(0, len(scans), batch)]

    def load(group):
        clouds = [load_scan_xyz(path) for _, path in group]
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        return np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32), offsets

    out = []
    for _, (points, offsets) in _read_ahead(load, batches):
        out.append(ops.scan_context(torch.from_numpy(points).cuda(), torch.from_numpy(offsets)))
    return [f for f, _ in scans], torch.cat(out)


def detect_sequence_loops(root, seq, threshold=LOOP_DEFAULTS['threshold'], exclude_recent=LOOP_DEFAULTS['exclude_recent'], raw=False,
                          batch=LOOP_DEFAULTS['batch'], log=print):
    """R/loops/%02d and R/loops/%02d.scores for one sequence -> [(query, candidate, distance, shift, yaw_deg)] (frame ids).  Scans
    are compared by their position in frame order, which is the frame id in a complete sequence."""
    from . import ops
    ids, desc = sequence_descriptors(root, seq, raw, batch)
    loops = list(zip(*ops.detect_loops(desc, threshold, exclude_recent)))
    gt = loop_ground_truth(root, seq)
    out_dir = osp.join(root, 'loops')
    os.makedirs(out_dir, exist_ok=True)
    out = []
    with open(osp.join(out_dir, '%02d' % seq), 'w') as f, open(osp.join(out_dir, '%02d.scores' % seq), 'w') as g:
        for q, c, d, s, yaw in loops:
            query, cand = ids[int(q)], ids[int(c)]
            out.append((query, cand, float(d), int(s), float(yaw)))
            f.write(format_pair_line(query, cand, loop_transform(gt, query, cand, int(s), desc.shape[2])))
            g.write(format_score_line(*out[-1]))
    log(f'sequence {seq:02d}: {len(ids)} scans, {len(out)} loops written to {osp.join(out_dir, "%02d" % seq)} with '
        + ('ground-truth poses' if gt is not None else 'yaw-only pose guesses (no poses / calib file)'))
    return out


def _parser():
    p = argparse.ArgumentParser(prog='python -m rdmnet_amd.prepare', description=__doc__.split('\n\n')[0])
    sub = p.add_subparsers(dest='command', required=True)
    d = sub.add_parser('downsample', help='raw scans -> downsampled_xyzi (0.3 m voxels, xyz + intensity)')
    d.add_argument('--dataset-root', required=True)
    d.add_argument('--sequences', type=int, nargs='+', default=list(range(11)))
    q = sub.add_parser('pairs', help='poses + raw scans -> icp{thres} pair lists with ICP-refined poses',
                       description='The default sequences are the reference\'s test split.  test_data_loader calibrates its '
                                   'neighbour limits on the train split, so a tree for it also needs --sequences 0 1 2 3 4 5.')
    q.add_argument('--dataset-root', required=True)
    q.add_argument('--sequences', type=int, nargs='+', default=[8, 9, 10],
                   help='default 8 9 10 (the test split); test_data_loader also needs 0 ... 5 (it calibrates on the train split)')
    q.add_argument('--thres', type=int, default=10, help='pair distance in metres (default 10)')
    q.add_argument('--max-iteration', type=int, default=5000)
    q.add_argument('--distance', type=float, default=0.5, help='ICP max correspondence distance in metres (default 0.5)')
    o = sub.add_parser('overlap', help='icp{distance} pair lists + downsampled_xyzi -> overlap{distance}: overlap and correspondences per pair')
    o.add_argument('--dataset-root', required=True)
    o.add_argument('--distance', type=int, default=10, help='the pair lists to read: icp{distance} (default 10)')
    o.add_argument('--radius', type=float, default=0.6, help='matching radius in metres (default 0.6)')
    o.add_argument('--workers', type=int, default=4, help='host threads that read scans ahead (default 4, at most 16)')
    lp = sub.add_parser('loops', help='scans -> loops/%%02d pair lists: Scan Context loop-closure detection, exhaustive on the GPU')
    lp.add_argument('--dataset-root', required=True)
    lp.add_argument('--sequences', type=int, nargs='+', default=list(range(11)))
    lp.add_argument('--threshold', type=float, default=LOOP_DEFAULTS['threshold'], help='a loop is accepted below this distance (default 0.13)')
    lp.add_argument('--exclude-recent', type=int, default=LOOP_DEFAULTS['exclude_recent'],
                    help='a candidate is at least this many frames older than its query (default 50; negative: any frame)')
    lp.add_argument('--raw', action='store_true', help='read sequences/%%02d/velodyne/*.bin instead of downsampled_xyzi/%%02d/*.npy')
    lp.add_argument('--batch', type=int, default=LOOP_DEFAULTS['batch'], help='scans per descriptor call (default 64)')
    return p


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    if not osp.isdir(a.dataset_root):
        p.error(f'--dataset-root {a.dataset_root} is not a directory')
    if a.command == 'overlap':
        if not a.radius > 0:
            p.error('--radius must be > 0')
        if not 1 <= a.workers <= 16:
            p.error('--workers must be 1 ... 16')
        for s in listed_sequences(a.dataset_root, a.distance):
            overlap_sequence(a.dataset_root, s, a.distance, a.radius, a.workers)
        return 0
    if any(s < 0 for s in a.sequences):
        p.error('sequences must be >= 0')
    if a.command == 'loops':
        if not a.threshold > 0:
            p.error('--threshold must be > 0')
        if not 1 <= a.batch <= 65535:
            p.error('--batch must be 1 ... 65535')
        for s in a.sequences:
            detect_sequence_loops(a.dataset_root, s, a.threshold, a.exclude_recent, a.raw, a.batch)
        return 0
    if a.command == 'pairs':
        if a.thres < 0:
            p.error('--thres must be >= 0')
        if a.max_iteration < 0:
            p.error('--max-iteration must be >= 0')
        if not a.distance > 0:
            p.error('--distance must be > 0')
        for s in a.sequences:
            generate_pairs(a.dataset_root, s, a.thres, a.max_iteration, a.distance)
    else:
        for s in a.sequences:
            downsample_sequence(a.dataset_root, s)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
