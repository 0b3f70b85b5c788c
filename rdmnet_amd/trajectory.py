"""Trajectories of a run over a sequence: the reference's chaining and absolute trajectory error, and the pose graph of a run.

    python -m rdmnet_amd.trajectory --features-root DIR [--optimize] [--line-process-weight MU] [--unit-information] [--out DIR]
                                  [--preconditioner {block_jacobi,chain}] [--linear-solver {pcg,direct}] [--covariance]
                                  [--loop-consistency] [--loop-gate D2]
                                  [--map-scans DATASET_ROOT [--map-raw] [--map-voxel 0.3] [--map-min-points 1]
                                   [--map-range LO HI] [--map-batch 64] [--map-sharpness [--map-sharpness-min-points 4]]
                                   [--map-min-scans 1]
                                   [--map-refine [--map-refine-sigma 0.02] [--map-refine-neighbors {1,7}] [--map-refine-iterations 30]
                                    [--map-refine-min-scans 1] [--map-refine-robust MU]]
                                   [--map-clean [--map-clean-max-d2 D] [--map-clean-sigma 0.02] [--map-clean-neighbors {1,7}]]
                                   [--map-save] [--map-prior FILE [--map-localize] [--map-prior-align [--map-prior-initial FILE]]]]

reads the `{seq}_{src}_{ref}.npz` pair files that `python -m rdmnet_amd.infer` wrote into DIR (ordered and filtered as
`python -m rdmnet_amd.eval` reads them) and, per sequence, chains the pair poses into a trajectory as
experiments/eval_pose_visualization_online.py:275-388 does (`cur_pose = cur_pose @ inv(est_transform)`), aligns it to the chained
ground truth with Umeyama and prints the absolute trajectory error of :173-212.  A pair whose src frame is the previous chain
pair's ref frame, and whose ref frame is new to the chain, continues the odometry chain (a certain edge of the pose graph; among
several such pairs the first in file order); every other pair file of the sequence is an uncertain (loop-closure) edge between
two frames of the chain.  With --optimize all sequences are optimised as one batch by
`ops.pose_graph_optimize` (--preconditioner chain selects its odometry-chain preconditioner, which suits exactly
these graphs; --linear-solver direct its direct sparse solve in place of the conjugate gradients) and the report is printed for the optimised trajectory too.  With --covariance
(which needs --optimize) every sequence's `pose graph:` line is followed by an `optimized uncertainty:` line -- the marginal covariance
of every optimised pose given frame 0 (`ops.pose_graph_marginals` at the optimised poses with the final line-process weights, pruned
edges at 0; one call per sequence): the median and the largest position sigma (root of the trace of the translation block, metres) and
rotation sigma (root of the trace of the rotation block, degrees) with the frames of the largest, or `not computed (K separator nodes,
limit 256)` for a sequence with more loop structure than the selected inversion takes -- and --out gets `{seq}_optimized_covariance.txt`,
one row of 36 numbers per frame of the chain (the 6 x 6 block of the right perturbation, rotation first; the first row zeros).  With
--loop-consistency (which needs the GPU but not --optimize) every sequence's `chained:` line is followed by a `loop consistency:` line:
the graph of the certain edges alone (the odometry chain) at the chained poses is asked how far every loop edge lies from the relative
pose it gives -- d2 = r^T (M + L^-1)^-1 r with M the covariance of the edge's residual under the chain (`ops.pose_graph_consistency`) and
L the edge's information -- and the line names the number of loop edges, the median and the largest d2 with its pair file; --out gets
`{seq}_loop_consistency.txt` (file name, s, t, d2 per loop edge).  --loop-gate D2 (needs --optimize, implies --loop-consistency, has no
default) leaves the loop edges with d2 > D2 (or without a d2) out of the optimised graph, the line ends with `, G above the gate D2`, and
the pose graph, uncertainty and map lines describe the graph that was optimised.  d2 is only as calibrated as the information matrices
are -- Open3D's scales with the number of correspondences -- so the gate is the user's number, not a chi-square quantile.  Without
--optimize and --loop-consistency no GPU is needed.  Everything here is numpy float64 on the host.  With --map-scans (and --out) the scans of every sequence's chain
frames are fused under the chained -- and with --optimize also the optimised -- poses into a voxel map on the GPU (`build_map`,
`ops.VoxelMap`) and written as `{seq}_{variant}_map.npy`; a better trajectory puts the same surfaces into
fewer voxels, so voxels and points per voxel of the two variants are a check of --optimize that needs no ground truth.  The
count is blind to small pose errors (they thicken the surfaces inside the voxels long before they spill into new ones), so with
--map-sharpness the map also keeps per-voxel second moments and every `map:` line is followed by a `sharpness:` line: the mean
plane thickness (root of the mean smallest covariance eigenvalue) and the mean map entropy over the voxels with at least
--map-sharpness-min-points points; lower is sharper for both.  With --map-refine the per-voxel Gaussians are also used to improve
the poses: every frame is registered against the map of the frames before it (`ops.VoxelMap.register`: point-to-distribution, the
NDT / voxelised-GICP family) and then fused into that map -- `refine_against_map` -- from the optimised poses with --optimize, else
the chained ones; the result is a third variant, `refined`, with its own error, pose file, map and sharpness lines.  With --map-min-scans N > 1 the map
also keeps in how many scans every voxel was seen (`ops.VoxelMap(observations=True)`) and every variant's map is pruned to the voxels
seen in at least N scans before anything is written or reported -- a moving object is in a voxel in one scan, static structure in
many --; a `persistent:` line after every `map:` line says what was kept.  --map-refine-min-scans N registers frame k >= N against
that pruned map instead of the full one.  --map-refine-robust MU (read by --map-refine and --map-localize; off by default) weights every
point-voxel pair of those registrations by (MU / (MU + d2))^2, d2 its squared Mahalanobis distance (`ops.VoxelMap.register`'s
robust_scale; 9 is a value to start from), so that an object which moved does not pull the poses, and a `robust weights:` line after the
`refined against the map` / `localized against` line says how many correspondences a frame has by weight.  With --map-clean (and --map-min-scans N >= 2, a finite --map-clean-max-d2 D, or both) every
point of every scan is judged by each variant's full map, before that prune (`clean_scans`, `ops.VoxelMap.query`): the scans are written
to `{seq}_{variant}_clean/` under their own names without the points that have no voxel, whose voxel was seen in fewer than N scans or that
lie further than D (squared Mahalanobis distance; the map then keeps second moments) from their voxel's Gaussian, and a `clean:` line after
the map's lines says what was dropped.  With --map-save every variant's full map, before that prune, is also written as
`{seq}_{variant}_map_state.npz` (`ops.VoxelMap.save`: the integers the map consists of; `ops.VoxelMap.load` gives the map back bit for
bit).  --map-prior FILE names such a file in the trajectory's world frame -- an earlier --map-save of the same sequence is one -- and
with it --map-clean judges the scans by that prior map instead of their own (--map-min-scans then counts the prior's scans; a scan that
is not in the map is what the distance test is for), and --map-localize registers every frame, independently, against the fixed prior
(`localize_against_map`): a variant `localized` with its own error, pose file and map lines.  With --map-prior-align the prior may
live in any frame: the map of the base variant (optimised with --optimize, else chained) is aligned to the prior on the voxel Gaussians
of both (`align_to_map`, `ops.VoxelMap.align`: voxelised GICP) from --map-prior-initial FILE (12 or 16 numbers, row-major: prior <-
trajectory) or the identity, the result T is written as `{seq}_prior_alignment.txt` and reported in an `aligned to the prior map` line
after the base variant's map lines, and T is applied only where the prior is touched: the prior is asked about T pose, and the poses
--map-localize gets back are moved by inv(T).  Every pose file, map and report stays in the trajectory's own frame."""
import argparse
import math
import os
import os.path as osp
import sys

import numpy as np

REFERENCE_KEYS = ('r_rmse', 'r_mean', 'rmse', 'mean')  # eval_absolute_error's dict, in its order


def chain_poses(transforms):
    """eval_pose_visualization_online.py:279,386-388: from the identity, cur_pose = cur_pose @ inv(est_transform) per pair, one
    pose per pair (the identity itself is not part of the trajectory).  -> float64 [n, 4, 4]."""
    cur = np.eye(4)
    out = np.zeros((len(transforms), 4, 4))
    for i, T in enumerate(transforms):
        cur = np.matmul(cur, np.linalg.inv(np.asarray(T, dtype=np.float64)))
        out[i] = cur
    return out


def umeyama_alignment(x, y, with_scale=False):
    """eval_pose_visualization_online.py:120-171 (Umeyama 1991): x, y [m, n] point sets -> (r, t, c) with y ~ c r x + t."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m, n = x.shape
    mean_x, mean_y = x.mean(axis=1), y.mean(axis=1)
    xc, yc = x - mean_x[:, None], y - mean_y[:, None]
    sigma_x = 1.0 / n * (np.linalg.norm(xc) ** 2)
    cov = np.zeros((m, m))
    for i in range(n):  # (the reference adds the outer products one by one)
        cov += np.outer(yc[:, i], xc[:, i])
    cov = np.multiply(1.0 / n, cov)
    u, d, v = np.linalg.svd(cov)
    s = np.eye(m)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[m - 1, m - 1] = -1
    r = u.dot(s).dot(v)
    c = 1 / sigma_x * np.trace(np.diag(d).dot(s)) if with_scale else 1.0
    t = mean_y - np.multiply(c, r.dot(mean_x))
    return r, t, c


def absolute_trajectory_error(traj, gt_traj):
    """eval_absolute_error (eval_pose_visualization_online.py:173-212) with gt_traj_inv = inv(gt_traj) (:591): the trajectory's
    positions are aligned to the ground truth's by umeyama_alignment (no scale), then per pose E = inv(gt) @ aligned.
    -> dict with the reference's four keys, literally: 'mean' and 'rmse' = round(., 3) * 100 of the mean of |translation
    component| over all 3 n components and of sqrt(sum of squared components / n) (centimetres); 'r_mean' = round(mean rotation
    angle in degrees, 2); 'r_rmse' = round(sqrt(TRANSLATION mean square), 2) -- the reference computes the rotation mean
    square and then takes the root of the translation's (:197-198).  Beside them: 'rotation_rmse_deg', the root of the rotation
    mean square (rounded to 2 decimals), and 'unrounded': {'mean', 'rmse' (metres), 'r_mean', 'rotation_rmse_deg' (degrees),
    'r_rmse' (the reference's quantity, = 'rmse')}."""
    traj, gt_traj = np.asarray(traj, dtype=np.float64), np.asarray(gt_traj, dtype=np.float64)
    r, t, _ = umeyama_alignment(traj[:, :3, 3].transpose((1, 0)), gt_traj[:, :3, 3].transpose((1, 0)))
    T = np.eye(4)
    T[:3, :3] = r
    T[:3, 3] = t
    err = np.matmul(np.linalg.inv(gt_traj), np.matmul(T, traj))
    traj_error = np.abs(err[:, :3, 3])
    mean = np.mean(traj_error)
    mse = np.sum(traj_error ** 2) / len(traj_error)
    rmse = np.sqrt(mse)
    tr = err[:, 0, 0] + err[:, 1, 1] + err[:, 2, 2]
    degrees = np.arccos(np.clip((tr - 1) / 2, -1, 1)) / math.pi * 180
    r_mean = np.mean(degrees)
    rot_rmse = np.sqrt(np.sum(degrees ** 2) / len(degrees))
    return {'r_rmse': round(rmse, 2), 'r_mean': round(r_mean, 2), 'rmse': round(rmse, 3) * 100, 'mean': round(mean, 3) * 100,
            'rotation_rmse_deg': round(rot_rmse, 2),
            'unrounded': {'mean': float(mean), 'rmse': float(rmse), 'r_mean': float(r_mean), 'r_rmse': float(rmse),
                          'rotation_rmse_deg': float(rot_rmse)}}


# ---- the pose graph of a run ------------------------------------------------------------------------------------------------

class TrajectoryError(Exception):
    pass


def read_sequences(features_root, unit_information=False):
    """-> {seq: dict(frames [n + 1] (the chain's frames, first the first pair's src), chain [(file, T, gt, information)],
    loops [(file, src, ref, T, information)])} in eval's file order."""
    from . import eval as ev
    _, todo = ev.list_pairs(features_root)
    seqs = {}
    for _, name, (seq, src, ref) in todo:
        with np.load(name) as z:
            T = np.asarray(z['estimated_transform'], dtype=np.float64)
            gt = np.asarray(z['transform'], dtype=np.float64) if 'transform' in z.files else None
            if unit_information:
                info = np.eye(6)
            elif 'information' in z.files:
                info = np.asarray(z['information'], dtype=np.float64)
            else:
                raise TrajectoryError(f"{name} has no 'information': write it with `python -m rdmnet_amd.infer --information`, or "
                                      "pass --unit-information")
        s = seqs.setdefault(seq, dict(frames=[], chain=[], loops=[]))
        if not s['chain'] or (src == s['frames'][-1] and ref not in s['frames']):
            if not s['chain']:
                s['frames'].append(src)
            s['frames'].append(ref)
            s['chain'].append((name, T, gt, info))
        else:
            s['loops'].append((name, src, ref, T, info))
    for seq, s in seqs.items():
        where = {f: i for i, f in reversed(list(enumerate(s['frames'])))}
        for name, src, ref, _, _ in s['loops']:
            for f in (src, ref):
                if f not in where:
                    raise TrajectoryError(f'{name}: frame {f} of sequence {seq} is not a frame of the odometry chain '
                                          f"({s['frames'][0]} ... {s['frames'][-1]})")
        s['where'] = where
    return seqs


def sequence_graph(s):
    """Nodes 0 .. n: the chain's frames, node 0 the first pair's src at the identity, the others chained (X_ref = X_src inv(T));
    edges (s = src node, t = ref node, T): first the chain's (certain), then the loops (uncertain).
    -> (nodes, edges, transforms, informations, uncertain, the file name of every edge)."""
    chained = chain_poses([T for _, T, _, _ in s['chain']])
    nodes = np.concatenate([np.eye(4)[None], chained])
    edges = [(i, i + 1) for i in range(len(s['chain']))] + [(s['where'][src], s['where'][ref]) for _, src, ref, _, _ in s['loops']]
    transforms = [T for _, T, _, _ in s['chain']] + [T for _, _, _, T, _ in s['loops']]
    infos = [L for _, _, _, L in s['chain']] + [L for _, _, _, _, L in s['loops']]
    uncertain = [0] * len(s['chain']) + [1] * len(s['loops'])
    names = [osp.basename(c[0]) for c in s['chain']] + [osp.basename(c[0]) for c in s['loops']]
    keep = [k for k, (a, b) in enumerate(edges) if a != b]  # (a loop pair inside one frame constrains nothing)
    pick = lambda v: [v[k] for k in keep]
    return (nodes, np.asarray(pick(edges), np.int64).reshape(-1, 2), np.asarray(pick(transforms)).reshape(-1, 4, 4),
            np.asarray(pick(infos)).reshape(-1, 6, 6), np.asarray(pick(uncertain), np.uint8), pick(names))


def uncertainty(graph, nodes, weights, pruned):
    """The marginal covariances [n, 6, 6] of one sequence's optimised poses (ops.pose_graph_marginals; pruned edges weigh 0), or the
    number of separator nodes when the graph needs more than the library's limit."""
    from . import _lib, ops
    edges = np.ascontiguousarray(graph[1], dtype=np.int64)
    limit = _lib.lib().rdm_pose_graph_direct_max_separator()
    need = _lib.lib().rdm_pose_graph_separator_host(len(nodes), len(edges), edges.ctypes.data, 0, 0)
    if need > limit:
        return int(need)
    res = ops.pose_graph_marginals(nodes, edges, graph[2], graph[3], np.where(pruned != 0, 0.0, weights))
    return res.covariances.cpu().numpy()


def uncertainty_line(seq, cov, limit=256):
    if isinstance(cov, int):
        return f'seq {seq} optimized uncertainty: not computed ({cov} separator nodes, limit {limit})'
    pos = np.sqrt(np.trace(cov[:, 3:, 3:], axis1=1, axis2=2))
    rot = np.degrees(np.sqrt(np.trace(cov[:, :3, :3], axis1=1, axis2=2)))
    return (f'seq {seq} optimized uncertainty: position sigma median {np.median(pos):.6g} m, max {pos.max():.6g} m at frame '
            f'{int(np.argmax(pos))}; rotation sigma median {np.median(rot):.6g} deg, max {rot.max():.6g} deg at frame {int(np.argmax(rot))}')


def loop_consistency(graph):
    """The squared Mahalanobis distance d2 [K] of every loop (uncertain) edge of one sequence's graph from the relative pose that the
    odometry chain alone gives, under the chain's uncertainty plus the edge's own (ops.pose_graph_consistency on the graph of the
    certain edges at the chained poses, every loop edge a pair with its transform and information), and the loop edges' numbers in the
    graph.  An edge whose d2 cannot be formed (an information matrix that is not positive definite) has NaN."""
    from . import ops
    nodes, edges, transforms, infos, uncertain = graph[:5]
    loops, chain = np.nonzero(uncertain != 0)[0], np.nonzero(uncertain == 0)[0]
    if len(loops) == 0:
        return np.zeros(0), loops
    res = ops.pose_graph_consistency(nodes, edges[chain], transforms[chain], infos[chain], pairs=edges[loops],
                                     pair_transforms=transforms[loops], pair_informations=infos[loops])
    return res.d2.cpu().numpy(), loops


def loop_consistency_line(seq, graph, d2, loops, gate=None):
    if len(loops) == 0:
        return f'seq {seq} loop consistency: 0 loop edges'
    worst = int(np.argmax(np.where(np.isnan(d2), np.inf, d2)))
    line = (f'seq {seq} loop consistency: {len(loops)} loop edges, d2 median {np.median(d2):.6g}, max {d2[worst]:.6g} '
            f'({graph[5][int(loops[worst])]})')
    if gate is not None:
        line += f', {int(np.count_nonzero(~(d2 <= gate)))} above the gate {gate:g}'
    return line


def without_edges(graph, drop):
    """The sequence graph without the edges numbered `drop`."""
    keep = np.setdiff1d(np.arange(len(graph[1])), drop)
    return (graph[0], graph[1][keep], graph[2][keep], graph[3][keep], graph[4][keep], [graph[5][int(k)] for k in keep])


def report_line(seq, what, err):
    return f'seq {seq} {what}: ' + ', '.join(f'{k}: {err[k]}' for k in REFERENCE_KEYS) + f", rotation_rmse_deg: {err['rotation_rmse_deg']}"


def write_kitti_poses(path, poses):
    """One line per pose: the 12 entries of its first three rows.  The command line writes one pose per FRAME of the chain, the first
    frame (the identity) included -- one line more than the reference's `traj` list, which the error report is computed on."""
    with open(path, 'w') as f:
        for X in poses:
            f.write(' '.join(f'{v:.9e}' for v in np.asarray(X)[:3].reshape(-1)) + '\n')


# ---- the map of a run ------------------------------------------------------------------------------------------------------

MAP_DEFAULTS = dict(voxel=0.3, min_points=1, batch=64, sharpness_min_points=4, min_scans=1)
REFINE_DEFAULTS = dict(sigma=0.02, neighbors=1, iterations=30, min_points=4, min_scans=1)
CLEAN_DEFAULTS = dict(sigma=0.02, neighbors=1, max_d2=math.inf)


def _read_batches(paths, batch):
    """Yields ((lo, hi), (points float32 [N, C], offsets int64 [hi - lo + 1])) for the scans paths[lo:hi], `batch` at a time, read on a
    background thread while the caller works on the batch before."""
    from . import prepare
    groups = [(i, min(i + int(batch), len(paths))) for i in range(0, len(paths), int(batch))]

    def load(group):
        clouds = [prepare.load_scan(paths[k]) for k in range(*group)]
        for k, c in zip(range(*group), clouds):
            if c.ndim != 2 or c.shape[1] != clouds[0].shape[-1]:
                raise TrajectoryError(f'{paths[k]}: shape {c.shape}, expected [N, {clouds[0].shape[-1]}] as the scans of its batch')
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        return np.concatenate(clouds), offsets

    return prepare._read_ahead(load, groups)


def build_map(paths, poses, voxel=MAP_DEFAULTS['voxel'], channels=None, min_range=0.0, max_range=math.inf, batch=MAP_DEFAULTS['batch'],
              capacity=1 << 20, device='cuda', moments=False, observations=False):
    """The scans `paths` (.npy float32 [N, C] or KITTI .bin [N, 4], read by prepare.load_scan) under `poses` ([n, 4, 4], world =
    pose @ point) fused into an ops.VoxelMap.  channels None: the columns of the first scan (at most 8).  `batch` scans are read on
    a background thread while the previous batch is on the GPU; a batch is one host-to-device copy and one integrate call.
    moments: keep the per-voxel second moments too (ops.VoxelMap(moments=True): extract_moments, sharpness); observations: and in how
    many scans every voxel was seen (ops.VoxelMap(observations=True): extract_observations, pruned; scan k has the id k).  A missing file is a TrajectoryError that names it (checked before anything is read)."""
    paths = list(paths)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(paths) != len(poses):
        raise ValueError(f'build_map: {len(paths)} scans and {len(poses)} poses')
    if int(batch) < 1:
        raise ValueError(f'build_map: batch must be >= 1, got {batch}')
    for path in paths:
        if not osp.isfile(path):
            raise TrajectoryError(f'{path}: no such scan file')
    import torch
    from . import ops
    vmap = None
    for group, (points, offsets) in _read_batches(paths, batch):
        if vmap is None:
            width = points.shape[1] if channels is None else int(channels)
            vmap = ops.VoxelMap(voxel, channels=min(width, 8), capacity=capacity, device=device, moments=moments,
                                observations=observations)
        if points.shape[1] < vmap.channels:
            raise TrajectoryError(f'{paths[group[0]]}: {points.shape[1]} columns, the map has {vmap.channels} channels')
        vmap.integrate((torch.from_numpy(points).to(vmap.device), torch.from_numpy(offsets)), poses[group[0]:group[1]], min_range,
                       max_range)
    if vmap is None:
        vmap = ops.VoxelMap(voxel, channels=4 if channels is None else int(channels), capacity=capacity, device=device, moments=moments,
                            observations=observations)
    return vmap


def map_line(seq, what, voxel, voxels, points, stats):
    per = f'{points / voxels:.2f}' if voxels else 'no'
    return (f'seq {seq} {what} map: {voxels} voxels at {voxel:g} m, {points} points, {per} points per voxel, skipped: '
            f"{stats['skipped_nonfinite']} non-finite, {stats['skipped_range']} out of range, {stats['out_of_extent']} out of extent")


def sharpness_line(seq, what, min_points, report):
    return (f"seq {seq} {what} sharpness: {report['qualified']} of {report['voxels']} voxels with >= {min_points} points, plane thickness "
            f"{report['plane_thickness'] * 1e3:.3f} mm, entropy {report['entropy']:.4f} ({report['degenerate']} degenerate)")


def persistent_line(seq, what, min_scans, kept, full, scans):
    """kept / full: the stats of the pruned and of the full map."""
    return (f"seq {seq} {what} persistent: {kept['occupied']} of {full['occupied']} voxels seen in >= {min_scans} scans, "
            f"{kept['integrated']} of {full['integrated']} points, {scans} scans")


def clean_scans(paths, poses, vmap, out_dir, *, min_scans=MAP_DEFAULTS['min_scans'], max_d2=math.inf, sigma=CLEAN_DEFAULTS['sigma'],
                min_points=MAP_DEFAULTS['min_points'], neighbors=CLEAN_DEFAULTS['neighbors'], min_range=0.0, max_range=math.inf,
                batch=MAP_DEFAULTS['batch']):
    """The scans `paths` (read as build_map reads them) under `poses` without the points that the map `vmap` does not call static
    (ops.VoxelMap.query: unmapped, in a voxel seen in fewer than min_scans scans, or further than max_d2 from its voxel's Gaussian):
    every scan's static rows, all columns, are written to out_dir under the scan's own file name and format.  The map is only read.
    -> the tallies int64 numpy [n, 8]: per scan the rows of each label of ops.MapQueryResult.LABELS, then the pairs."""
    paths = list(paths)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(paths) != len(poses):
        raise ValueError(f'clean_scans: {len(paths)} scans and {len(poses)} poses')
    if int(batch) < 1:
        raise ValueError(f'clean_scans: batch must be >= 1, got {batch}')
    names = [osp.basename(p) for p in paths]
    if len(set(names)) != len(names):
        raise ValueError('clean_scans: two scans have the same file name')
    for path in paths:
        if not osp.isfile(path):
            raise TrajectoryError(f'{path}: no such scan file')
    import torch
    from . import ops
    os.makedirs(out_dir, exist_ok=True)
    static = ops.MapQueryResult.LABELS.index('static')
    tallies = np.zeros((len(paths), 8), np.int64)
    for (lo, hi), (points, offsets) in _read_batches(paths, batch):
        if points.shape[1] < vmap.channels:
            raise TrajectoryError(f'{paths[lo]}: {points.shape[1]} columns, the map has {vmap.channels} channels')
        res = vmap.query((torch.from_numpy(points).to(vmap.device), torch.from_numpy(offsets)), poses[lo:hi], sigma=sigma,
                         min_points=min_points, neighbors=neighbors, min_scans=min_scans, max_d2=max_d2, min_range=min_range,
                         max_range=max_range, outputs=('labels', 'tallies'))
        tallies[lo:hi] = res.tallies.cpu().numpy()
        keep = res.labels.cpu().numpy() == static
        for k in range(lo, hi):
            rows = points[offsets[k - lo]:offsets[k - lo + 1]][keep[offsets[k - lo]:offsets[k - lo + 1]]]
            if names[k].endswith('.bin'):
                rows.astype(np.float32).tofile(osp.join(out_dir, names[k]))
            else:
                np.save(osp.join(out_dir, names[k]), rows)
    return tallies


def prior_words(prior):
    """prior: dict(name, voxels, voxel, scans, moments) of a --map-prior map, as the lines name it."""
    return (f"the prior map {prior['name']} ({prior['voxels']} voxels at {prior['voxel']:g} m, {prior['scans']} scans"
            + ('' if prior['moments'] else ', no moments: Sigma = sigma^2 I') + ')')


def clean_line(seq, what, tallies, min_scans, max_d2, prior=None):
    """prior: None when the scans were judged by their own map, else what prior_words takes."""
    t = np.asarray(tallies, np.int64).reshape(-1, 8).sum(0)
    return (f'seq {seq} {what} clean: {t[6]} of {t[:7].sum()} points kept in {len(tallies)} scans, dropped: {t[3]} unmapped, '
            f'{t[4]} transient (< {min_scans} scans), {t[5]} off surface (d2 > {max_d2:g}), {t[:3].sum()} gated'
            + ('' if prior is None else ', judged by ' + prior_words(prior)))


def refine_against_map(paths, poses, voxel=MAP_DEFAULTS['voxel'], channels=None, min_range=0.0, max_range=math.inf,
                       sigma=REFINE_DEFAULTS['sigma'], neighbors=REFINE_DEFAULTS['neighbors'], max_iteration=REFINE_DEFAULTS['iterations'],
                       min_points=REFINE_DEFAULTS['min_points'], capacity=1 << 20, device='cuda', min_scans=REFINE_DEFAULTS['min_scans'],
                       observations=False, robust_scale=None):
    """Sequential scan-to-map refinement of the trajectory `poses` ([n, 4, 4]) of the scans `paths` (as build_map reads them): frame
    0 keeps its pose and is integrated into a map with moments; every later frame k starts from refined[k - 1] inv(poses[k - 1])
    poses[k] -- the previous frame's correction carried forward --, is registered against the map so far (ops.VoxelMap.register)
    and integrated under the result.  A degenerate frame (status 2: no correspondence, or a singular system) keeps its initial
    pose.  min_scans N > 1: frame k >= N is registered against vmap.pruned(N), the voxels seen in at least N of the frames before it
    (earlier frames against the full map); every frame is still integrated into the full map, which then keeps observations, as it does
    with observations=True.  robust_scale: None, or ops.VoxelMap.register's (every pair weighted by its Mahalanobis distance, so that
    what moves between the frames does not pull the poses); the dict then also holds weights [n], the correspondences by weight.  The
    scans are read on a background thread, one ahead.  -> (refined float64 [n, 4, 4], the ops.VoxelMap of all frames
    under the refined poses, dict(frames, iterations [n], correspondences [n], status [n], degenerate)); frame 0 has status -1."""
    paths = list(paths)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(paths) != len(poses):
        raise ValueError(f'refine_against_map: {len(paths)} scans and {len(poses)} poses')
    min_scans = int(min_scans)
    if min_scans < 1:
        raise ValueError(f'refine_against_map: min_scans must be >= 1, got {min_scans}')
    kind = dict(moments=True, observations=bool(observations) or min_scans > 1)
    for path in paths:
        if not osp.isfile(path):
            raise TrajectoryError(f'{path}: no such scan file')
    import torch
    from . import ops, prepare
    refined = poses.copy()
    n = len(paths)
    iterations, corr, status = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    weights = np.zeros(n, np.float64)
    vmap = None
    for k, cloud in prepare._read_ahead(lambda k: prepare.load_scan(paths[k]), list(range(n))):
        if cloud.ndim != 2 or cloud.shape[1] < 3:
            raise TrajectoryError(f'{paths[k]}: shape {cloud.shape}, expected [N, >= 3]')
        if vmap is None:
            width = cloud.shape[1] if channels is None else int(channels)
            vmap = ops.VoxelMap(voxel, channels=min(width, 8), capacity=capacity, device=device, **kind)
        if cloud.shape[1] < vmap.channels:
            raise TrajectoryError(f'{paths[k]}: {cloud.shape[1]} columns, the map has {vmap.channels} channels')
        points = torch.from_numpy(np.ascontiguousarray(cloud)).to(vmap.device)
        if k > 0:
            init = refined[k - 1] @ np.linalg.inv(poses[k - 1]) @ poses[k]
            target = vmap.pruned(min_scans) if min_scans > 1 and k >= min_scans else vmap
            res = target.register([points], init[None], sigma=sigma, min_points=min_points, neighbors=neighbors, max_iteration=max_iteration,
                                min_range=min_range, max_range=max_range, robust_scale=robust_scale)
            iterations[k], corr[k], status[k] = torch.stack([res.iterations, res.num_correspondences, res.status]).cpu().numpy()[:, 0]
            if robust_scale is not None:
                weights[k] = float(res.weight_sum[0])
            refined[k] = init if status[k] == 2 else res.transformations[0].cpu().numpy()
        vmap.integrate([points], refined[k][None], min_range, max_range)
    if vmap is None:
        vmap = ops.VoxelMap(voxel, channels=4 if channels is None else int(channels), capacity=capacity, device=device, **kind)
    stats = dict(frames=n, iterations=iterations, correspondences=corr, status=status, degenerate=int((status == 2).sum()))
    if robust_scale is not None:
        stats['weights'] = weights
    return refined, vmap, stats


def refine_line(seq, stats):
    moved = max(stats['frames'] - 1, 1)
    return (f"seq {seq} refined against the map: {stats['frames']} frames, {stats['iterations'].sum() / moved:.2f} iterations and "
            f"{stats['correspondences'].sum() / moved:.0f} correspondences per frame, {stats['degenerate']} degenerate frames")


def robust_line(seq, what, scale, stats):
    """what: 'refined' (per registered frame: all but the first) or 'localized' (per frame); stats: with `weights`."""
    frames = max(stats['frames'] - 1 if what == 'refined' else stats['frames'], 1)
    return (f"seq {seq} {what} robust weights: scale {scale:g}, {stats['weights'].sum() / frames:.1f} of "
            f"{stats['correspondences'].sum() / frames:.0f} correspondences per frame by weight")


def localize_against_map(paths, poses, vmap, *, sigma=REFINE_DEFAULTS['sigma'], neighbors=REFINE_DEFAULTS['neighbors'],
                         max_iteration=REFINE_DEFAULTS['iterations'], min_points=REFINE_DEFAULTS['min_points'], min_range=0.0,
                         max_range=math.inf, batch=MAP_DEFAULTS['batch'], robust_scale=None):
    """Every scan of `paths` (as build_map reads them) registered from its pose in `poses` ([n, 4, 4]) against the fixed map `vmap` (an
    ops.VoxelMap with moments, such as ops.VoxelMap.load gives; ops.VoxelMap.register).  The frames are independent: `batch` scans are
    one register call, and nothing is integrated -- the map is only read.  A degenerate frame (status 2) keeps its pose.  robust_scale:
    None, or ops.VoxelMap.register's; the dict then also holds weights [n], the correspondences by weight.  -> (localized
    float64 [n, 4, 4], dict(frames, iterations [n], correspondences [n], status [n], degenerate))."""
    paths = list(paths)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(paths) != len(poses):
        raise ValueError(f'localize_against_map: {len(paths)} scans and {len(poses)} poses')
    if int(batch) < 1:
        raise ValueError(f'localize_against_map: batch must be >= 1, got {batch}')
    if not vmap.moments:
        raise ValueError('localize_against_map: the map has no moments')
    for path in paths:
        if not osp.isfile(path):
            raise TrajectoryError(f'{path}: no such scan file')
    import torch
    n = len(paths)
    localized = poses.copy()
    iterations, corr, status = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    weights = np.zeros(n, np.float64)
    for (lo, hi), (points, offsets) in _read_batches(paths, batch):
        if points.shape[1] < vmap.channels:
            raise TrajectoryError(f'{paths[lo]}: {points.shape[1]} columns, the map has {vmap.channels} channels')
        res = vmap.register((torch.from_numpy(points).to(vmap.device), torch.from_numpy(offsets)), poses[lo:hi], sigma=sigma,
                            min_points=min_points, neighbors=neighbors, max_iteration=max_iteration, min_range=min_range,
                            max_range=max_range, robust_scale=robust_scale)
        iterations[lo:hi], corr[lo:hi], status[lo:hi] = torch.stack([res.iterations, res.num_correspondences, res.status]).cpu().numpy()
        if robust_scale is not None:
            weights[lo:hi] = res.weight_sum.cpu().numpy()
        moved = status[lo:hi] != 2
        localized[lo:hi][moved] = res.transformations.cpu().numpy()[moved]
    stats = dict(frames=n, iterations=iterations, correspondences=corr, status=status, degenerate=int((status == 2).sum()))
    if robust_scale is not None:
        stats['weights'] = weights
    return localized, stats


def localize_line(seq, stats, prior):
    frames = max(stats['frames'], 1)
    return (f"seq {seq} localized against {prior_words(prior)}: {stats['frames']} frames, {stats['iterations'].sum() / frames:.2f} "
            f"iterations and {stats['correspondences'].sum() / frames:.0f} correspondences per frame, {stats['degenerate']} degenerate frames")


def read_transform(path):
    """A text file of 12 or 16 numbers, row-major -> float64 [4, 4] (12: the last row is 0 0 0 1)."""
    try:
        with open(path) as f:
            values = [float(v) for v in f.read().split()]
    except FileNotFoundError:
        raise TrajectoryError(f'{path}: no such file')
    except ValueError as e:
        raise TrajectoryError(f'{path}: not a text file of numbers ({e})')
    if len(values) not in (12, 16) or not np.isfinite(values).all():
        raise TrajectoryError(f'{path}: expected 12 or 16 finite numbers (a row-major 3x4 or 4x4 transform), got {len(values)}')
    T = np.eye(4)
    T.reshape(-1)[:len(values)] = values
    if T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise TrajectoryError(f'{path}: the last row of a 4x4 transform must be 0 0 0 1')
    return T


def align_to_map(paths, poses, prior, initial=None, *, voxel=MAP_DEFAULTS['voxel'], sigma=REFINE_DEFAULTS['sigma'],
                 neighbors=REFINE_DEFAULTS['neighbors'], max_iteration=REFINE_DEFAULTS['iterations'], min_points=REFINE_DEFAULTS['min_points'],
                 source_min_points=REFINE_DEFAULTS['min_points'], min_range=0.0, max_range=math.inf, batch=MAP_DEFAULTS['batch']):
    """Where the trajectory `poses` ([n, 4, 4]) of the scans `paths` sits in the frame of the map `prior` (an ops.VoxelMap with moments):
    the scans are fused under the poses into a map with moments at `voxel` (build_map) and that map is aligned, as the source, to the
    prior (ops.VoxelMap.align) from `initial` ([4, 4], prior <- trajectory; None: the identity).  Both maps are only read once built.
    -> (T float64 [4, 4], dict(status, iterations, correspondences, cost, matched, voxels, moved_m, moved_deg)): matched / voxels are
    the correspondences and the source voxels of one more evaluation at T with the voxel's own cell alone; moved: from `initial` to T.
    A degenerate alignment (status 2) returns `initial`."""
    if not prior.moments:
        raise ValueError('align_to_map: the prior has no moments')
    T0 = np.eye(4) if initial is None else np.asarray(initial, dtype=np.float64).reshape(4, 4)
    source = build_map(paths, poses, voxel=voxel, channels=prior.channels, min_range=min_range, max_range=max_range, batch=batch,
                       device=prior.device, moments=True)
    res = prior.align([source], T0[None], sigma=sigma, min_points=min_points, source_min_points=source_min_points, neighbors=neighbors,
                      max_iteration=max_iteration)
    status, iterations, corr = (int(v[0]) for v in (res.status, res.iterations, res.num_correspondences))
    T = T0.copy() if status == 2 else res.transformations[0].cpu().numpy()
    own = prior.align([source], T[None], sigma=sigma, min_points=min_points, source_min_points=source_min_points, neighbors=1,
                      max_iteration=0)
    E = T[:3, :3] @ T0[:3, :3].T
    return T, dict(status=status, iterations=iterations, correspondences=corr, cost=float(res.cost[0]),
                   matched=int(own.num_correspondences[0]), voxels=int(own.num_points[0]),
                   moved_m=float(np.linalg.norm(T[:3, 3] - T0[:3, 3])),
                   moved_deg=float(np.degrees(np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0)))))


def align_line(seq, what, prior, stats):
    """prior: what prior_words takes; stats: align_to_map's."""
    from .ops import MapRegistrationResult
    return (f"seq {seq} {what} aligned to the prior map {prior['name']}: {stats['matched']} of {stats['voxels']} voxels matched, "
            f"{stats['correspondences']} correspondences, {stats['iterations']} iterations, cost {stats['cost']:.6g}, moved "
            f"{stats['moved_m']:.3f} m / {stats['moved_deg']:.3f} deg ({MapRegistrationResult.STATUS[stats['status']]})")


def load_prior(args):
    """(the ops.VoxelMap of --map-prior, what prior_words takes), loaded once per run from the state that map_paths read; (None, None)
    without the flag."""
    if getattr(args, 'map_prior', None) is None:
        return None, None
    if getattr(args, 'map_prior_loaded', None) is None:
        from . import ops
        vmap = ops.VoxelMap.from_state(args.map_prior_state)
        args.map_prior_loaded = (vmap, dict(name=osp.basename(args.map_prior), voxels=len(args.map_prior_state['keys']), voxel=vmap.voxel,
                                            scans=vmap.num_scans, moments=vmap.moments))
    return args.map_prior_loaded


def write_map(args, seq, what, paths, poses, emit, vmap=None, to_prior=None):
    """vmap: the map of these scans under these poses when the caller has built it already (the refinement's); to_prior: the
    --map-prior-align transform (prior <- trajectory), under which the prior judges the scans."""
    lo, hi = args.map_range if args.map_range else (0.0, math.inf)
    sharpness = bool(getattr(args, 'map_sharpness', False))
    min_scans = getattr(args, 'map_min_scans', None) or MAP_DEFAULTS['min_scans']
    clean = bool(getattr(args, 'map_clean', False))
    max_d2 = getattr(args, 'map_clean_max_d2', None) if clean else None
    max_d2 = CLEAN_DEFAULTS['max_d2'] if max_d2 is None else max_d2
    judge, prior = load_prior(args) if clean else (None, None)
    if vmap is None:
        vmap = build_map(paths, poses, voxel=args.map_voxel, min_range=lo, max_range=hi, batch=args.map_batch,
                         moments=sharpness or (math.isfinite(max_d2) and judge is None), observations=min_scans > 1)
    if getattr(args, 'map_save', False):  # the full map
        vmap.save(osp.join(args.out, f'{seq}_{what}_map_state.npz'))
    if clean:  # the scans against the full map, or against the prior
        asked = poses if judge is None or to_prior is None else to_prior @ np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        tallies = clean_scans(paths, asked, vmap if judge is None else judge, osp.join(args.out, f'{seq}_{what}_clean'), min_scans=min_scans, max_d2=max_d2,
                              sigma=args.map_clean_sigma, min_points=args.map_min_points, neighbors=args.map_clean_neighbors,
                              min_range=lo, max_range=hi, batch=args.map_batch)
    if min_scans > 1:  # everything below describes the pruned map
        full, scans = vmap.stats(), vmap.num_scans
        vmap = vmap.pruned(min_scans)
    points, counts, _ = vmap.extract(args.map_min_points)
    points, counts = points.cpu().numpy(), counts.cpu().numpy()
    np.save(osp.join(args.out, f'{seq}_{what}_map.npy'), np.concatenate([points, counts[:, None].astype(np.float32)], 1))
    emit(map_line(seq, what, args.map_voxel, len(counts), int(counts.sum(dtype=np.int64)), vmap.stats()))
    if min_scans > 1:
        emit(persistent_line(seq, what, min_scans, vmap.stats(), full, scans))
    if sharpness:
        emit(sharpness_line(seq, what, args.map_sharpness_min_points, vmap.sharpness(args.map_sharpness_min_points)))
    if clean:
        emit(clean_line(seq, what, tallies, min_scans, max_d2, prior))


def map_paths(args, seqs):
    """{seq: the scan file of every chain frame}, after the checks that need no GPU."""
    refine, localize = bool(getattr(args, 'map_refine', False)), bool(getattr(args, 'map_localize', False))
    prior = getattr(args, 'map_prior', None)
    align, initial = bool(getattr(args, 'map_prior_align', False)), getattr(args, 'map_prior_initial', None)
    if initial is not None and not align:
        raise TrajectoryError('--map-prior-initial needs --map-prior-align (it is where the alignment to the prior map starts)')
    if align and not (prior and getattr(args, 'map_scans', None) and args.out):
        raise TrajectoryError("--map-prior-align needs --map-prior, --map-scans and --out (the map of the scans is aligned to the prior map)")
    if getattr(args, 'map_save', False) and not (getattr(args, 'map_scans', None) and args.out):
        raise TrajectoryError('--map-save needs --map-scans and --out (the maps of the scans are written to --out)')
    if localize and not (prior and getattr(args, 'map_scans', None) and args.out):
        raise TrajectoryError('--map-localize needs --map-prior, --map-scans and --out (the frames are registered against the prior map)')
    if prior and not (localize or align or getattr(args, 'map_clean', False)):
        raise TrajectoryError('--map-prior needs --map-clean or --map-localize (the prior judges the scans or localises the frames)')
    if refine and not (getattr(args, 'map_scans', None) and args.out):
        raise TrajectoryError('--map-refine needs --map-scans and --out (the frames are registered against the map of the scans)')
    if not refine:
        for flag, key in (('--map-refine-sigma', 'sigma'), ('--map-refine-neighbors', 'neighbors'), ('--map-refine-iterations', 'iterations'),
                          ('--map-refine-min-scans', 'min_scans')):
            if getattr(args, 'map_refine_' + key, None) not in (None, REFINE_DEFAULTS[key]) and not ((localize or align) and key != 'min_scans'):
                raise TrajectoryError(f'{flag} needs --map-refine' + ('' if key == 'min_scans' else ' (or --map-localize)'))
        if getattr(args, 'map_refine_robust', None) is not None and not localize:
            raise TrajectoryError('--map-refine-robust needs --map-refine (or --map-localize)')
    if (refine or localize or align) and (not (args.map_refine_sigma > 0 and math.isfinite(args.map_refine_sigma)) or args.map_refine_iterations < 0):
        raise TrajectoryError('--map-refine-sigma must be > 0 and --map-refine-iterations >= 0')
    if refine and getattr(args, 'map_refine_min_scans', REFINE_DEFAULTS['min_scans']) < 1:
        raise TrajectoryError(f'--map-refine-min-scans must be >= 1, got {args.map_refine_min_scans}')
    if not getattr(args, 'map_clean', False):
        for flag, key in (('--map-clean-max-d2', 'max_d2'), ('--map-clean-sigma', 'sigma'), ('--map-clean-neighbors', 'neighbors')):
            if getattr(args, 'map_clean_' + key, None) not in (None, CLEAN_DEFAULTS[key]):
                raise TrajectoryError(f'{flag} needs --map-clean')
    elif not (getattr(args, 'map_scans', None) and args.out):
        raise TrajectoryError('--map-clean needs --map-scans and --out (the scans are judged by their map and written to --out)')
    elif not (args.map_clean_sigma > 0 and math.isfinite(args.map_clean_sigma)) or not args.map_clean_max_d2 >= 0:
        raise TrajectoryError('--map-clean-sigma must be > 0 and --map-clean-max-d2 >= 0')
    elif not (getattr(args, 'map_min_scans', MAP_DEFAULTS['min_scans']) >= 2 or math.isfinite(args.map_clean_max_d2)):
        raise TrajectoryError('--map-clean needs a criterion: --map-min-scans N >= 2 (drop what was seen in fewer scans) or a finite '
                              '--map-clean-max-d2 D (drop what lies off the surface)')
    if not getattr(args, 'map_scans', None):
        if getattr(args, 'map_min_scans', None) not in (None, MAP_DEFAULTS['min_scans']):
            raise TrajectoryError('--map-min-scans needs --map-scans (the voxels are counted over the scans of the map)')
        if getattr(args, 'map_sharpness', False):
            raise TrajectoryError('--map-sharpness needs --map-scans (the report is taken over the map of the scans)')
        if getattr(args, 'map_sharpness_min_points', None) not in (None, MAP_DEFAULTS['sharpness_min_points']):
            raise TrajectoryError('--map-sharpness-min-points needs --map-scans and --map-sharpness')
        return None
    if prior:
        from . import ops
        try:
            args.map_prior_state, args.map_prior_loaded = ops.read_state(prior), None
        except FileNotFoundError:
            raise TrajectoryError(f'--map-prior {prior}: no such file')
        except Exception as e:  # (not a zip archive, not a state, records that no map holds: read_state says which)
            raise TrajectoryError(f'--map-prior {prior}: cannot be read as a voxel map state ({e})')
        if localize and args.map_prior_state.get('moments') is None:
            raise TrajectoryError(f'--map-localize needs a prior with moments; --map-prior {prior} has none (save it from a run with '
                                  '--map-sharpness or a finite --map-clean-max-d2)')
        if align and args.map_prior_state.get('moments') is None:
            raise TrajectoryError(f'--map-prior-align needs a prior with moments; --map-prior {prior} has none (save it from a run with '
                                  '--map-sharpness or a finite --map-clean-max-d2)')
        args.map_prior_start = read_transform(initial) if initial is not None else None
        if getattr(args, 'map_clean', False) and getattr(args, 'map_min_scans', MAP_DEFAULTS['min_scans']) >= 2 \
                and args.map_prior_state.get('observations') is None:
            raise TrajectoryError(f'--map-min-scans {args.map_min_scans} with --map-clean counts the scans of the prior; --map-prior {prior} '
                                  'has no observations (save it from a run with --map-min-scans N >= 2)')
    if getattr(args, 'map_sharpness', False) and args.map_sharpness_min_points < 2:
        raise TrajectoryError(f'--map-sharpness-min-points must be >= 2 (a covariance needs two points), got {args.map_sharpness_min_points}')
    if getattr(args, 'map_min_scans', MAP_DEFAULTS['min_scans']) < 1:
        raise TrajectoryError(f'--map-min-scans must be >= 1, got {args.map_min_scans}')
    if not args.out:
        raise TrajectoryError('--map-scans needs --out (the directory the maps are written to)')
    if not (args.map_voxel > 0 and math.isfinite(args.map_voxel)) or args.map_min_points < 1 or args.map_batch < 1:
        raise TrajectoryError('--map-voxel must be > 0, --map-min-points and --map-batch >= 1')
    if args.map_range and not 0.0 <= args.map_range[0] <= args.map_range[1]:
        raise TrajectoryError(f'--map-range LO HI needs 0 <= LO <= HI, got {args.map_range[0]} {args.map_range[1]}')
    from . import prepare
    out = {}
    for seq, s in seqs.items():
        out[seq] = [prepare.scan_path(args.map_scans, seq, f, args.map_raw) for f in s['frames']]
        for path in out[seq]:
            if not osp.isfile(path):
                raise TrajectoryError(f'{path}: no such scan file (frame of sequence {seq}; --map-scans {args.map_scans}'
                                      + ('' if args.map_raw else ', --map-raw reads sequences/%02d/velodyne/*.bin') + ')')
    return out


def run(args, emit=print):
    covariance = bool(getattr(args, 'covariance', False))
    if covariance and not args.optimize:
        raise TrajectoryError('--covariance needs --optimize')
    gate = getattr(args, 'loop_gate', None)
    if gate is not None and not args.optimize:
        raise TrajectoryError('--loop-gate needs --optimize')
    seqs = read_sequences(args.features_root, args.unit_information)
    graphs = {seq: sequence_graph(s) for seq, s in seqs.items()}
    consistency = {}
    if getattr(args, 'loop_consistency', False) or gate is not None:
        for seq in graphs:  # (before anything is optimised: the gate decides what is)
            d2, loops = loop_consistency(graphs[seq])
            consistency[seq] = (loop_consistency_line(seq, graphs[seq], d2, loops, gate),
                                [(graphs[seq][5][int(e)], *graphs[seq][1][int(e)], v) for e, v in zip(loops, d2)])
            if gate is not None:
                graphs[seq] = without_edges(graphs[seq], loops[~(d2 <= gate)])
    scans = map_paths(args, seqs)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    gts = {}
    align = bool(getattr(args, 'map_prior_align', False))
    solved, aligned = [], {}

    def optimised():
        """The pose graphs of all sequences, optimised once -> (res, nodes, pruned, order, noff, eoff)."""
        if not solved:
            from . import ops
            order = list(graphs)
            noff = np.cumsum([0] + [len(graphs[q][0]) for q in order])
            eoff = np.cumsum([0] + [len(graphs[q][1]) for q in order])
            cat = lambda k, shape: np.concatenate([graphs[q][k].reshape(shape) for q in order]) if order else np.zeros(shape[1:])
            res = ops.pose_graph_optimize(cat(0, (-1, 4, 4)), cat(1, (-1, 2)), cat(2, (-1, 4, 4)), cat(3, (-1, 6, 6)), cat(4, (-1,)),
                                          line_process_weight=args.line_process_weight, edge_prune_threshold=args.edge_prune_threshold,
                                          max_iterations=args.max_iterations, graph_node_offsets=noff, graph_edge_offsets=eoff,
                                          preconditioner=getattr(args, 'preconditioner', 'block_jacobi'),
                                          linear_solver=getattr(args, 'linear_solver', 'pcg'))
            solved.append((res, res.nodes.cpu().numpy(), res.pruned.cpu().numpy(), order, noff, eoff))
        return solved[0]

    def to_prior(seq):
        """--map-prior-align: (T, its line) of the sequence's base variant, found when the prior is first touched; else (None, None)."""
        if not align:
            return None, None
        if seq not in aligned:
            if args.optimize:
                _, nodes, _, order, noff, _ = optimised()
                g = order.index(seq)
                base, what = nodes[noff[g]:noff[g + 1]], 'optimized'
            else:
                base, what = graphs[seq][0], 'chained'
            lo, hi = args.map_range if args.map_range else (0.0, math.inf)
            vmap, prior = load_prior(args)
            T, stats = align_to_map(scans[seq], base, vmap, args.map_prior_start, voxel=args.map_voxel, sigma=args.map_refine_sigma,
                                    neighbors=args.map_refine_neighbors, max_iteration=args.map_refine_iterations, min_range=lo,
                                    max_range=hi, batch=args.map_batch)
            if stats['status'] == 2:
                raise TrajectoryError(f"seq {seq}: the alignment of the {what} map to the prior map {prior['name']} is degenerate "
                                      f"({stats['correspondences']} correspondences): give a better start with --map-prior-initial")
            np.savetxt(osp.join(args.out, f'{seq}_prior_alignment.txt'), T, fmt='%.9e')
            aligned[seq] = (T, align_line(seq, what, prior, stats))
        return aligned[seq]

    for seq, s in seqs.items():
        traj = graphs[seq][0][1:]
        if all(gt is not None for _, _, gt, _ in s['chain']):
            gts[seq] = chain_poses([gt for _, _, gt, _ in s['chain']])
            emit(report_line(seq, 'chained', absolute_trajectory_error(traj, gts[seq])))
        else:
            emit(f'seq {seq} chained: no ground truth in the pair files')
        if seq in consistency:
            emit(consistency[seq][0])
            if args.out:
                with open(osp.join(args.out, f'{seq}_loop_consistency.txt'), 'w') as f:
                    for name, a, b, v in consistency[seq][1]:
                        f.write(f'{name} {a} {b} {v:.9e}\n')
        if args.out:
            write_kitti_poses(osp.join(args.out, f'{seq}_chained.txt'), graphs[seq][0])
        if scans:
            write_map(args, seq, 'chained', scans[seq], graphs[seq][0], emit, to_prior=to_prior(seq)[0])
            if align and not args.optimize:
                emit(to_prior(seq)[1])

    def refine(seq, base):
        lo, hi = args.map_range if args.map_range else (0.0, math.inf)
        refined, vmap, stats = refine_against_map(scans[seq], base, voxel=args.map_voxel, min_range=lo, max_range=hi,
                                                  sigma=args.map_refine_sigma, neighbors=args.map_refine_neighbors,
                                                  max_iteration=args.map_refine_iterations,
                                                  min_scans=getattr(args, 'map_refine_min_scans', None) or REFINE_DEFAULTS['min_scans'],
                                                  observations=(getattr(args, 'map_min_scans', None) or 1) > 1,
                                                  robust_scale=getattr(args, 'map_refine_robust', None))
        if seq in gts:
            emit(report_line(seq, 'refined', absolute_trajectory_error(refined[1:], gts[seq])))
        emit(refine_line(seq, stats))
        if 'weights' in stats:
            emit(robust_line(seq, 'refined', args.map_refine_robust, stats))
        write_kitti_poses(osp.join(args.out, f'{seq}_refined.txt'), refined)
        write_map(args, seq, 'refined', scans[seq], refined, emit, vmap=vmap, to_prior=to_prior(seq)[0])

    def localize(seq, base):
        lo, hi = args.map_range if args.map_range else (0.0, math.inf)
        vmap, prior = load_prior(args)
        T = to_prior(seq)[0]
        localized, stats = localize_against_map(scans[seq], base if T is None else T @ base, vmap, sigma=args.map_refine_sigma, neighbors=args.map_refine_neighbors,
                                                max_iteration=args.map_refine_iterations, min_range=lo, max_range=hi,
                                                batch=args.map_batch, robust_scale=getattr(args, 'map_refine_robust', None))
        if T is not None:  # back into the trajectory's frame; a degenerate frame keeps its pose
            localized = np.where((stats['status'] == 2)[:, None, None], base, np.linalg.inv(T) @ localized)
        if seq in gts:
            emit(report_line(seq, 'localized', absolute_trajectory_error(localized[1:], gts[seq])))
        emit(localize_line(seq, stats, prior))
        if 'weights' in stats:
            emit(robust_line(seq, 'localized', args.map_refine_robust, stats))
        write_kitti_poses(osp.join(args.out, f'{seq}_localized.txt'), localized)
        write_map(args, seq, 'localized', scans[seq], localized, emit, to_prior=T)

    if not args.optimize:
        for seq in seqs:
            if getattr(args, 'map_refine', False):
                refine(seq, graphs[seq][0])
            if getattr(args, 'map_localize', False):
                localize(seq, graphs[seq][0])
        return None
    if not graphs:
        raise TrajectoryError(f'{args.features_root}: no pair files to optimise')
    res, nodes, pruned, order, noff, eoff = optimised()
    for g, seq in enumerate(order):
        traj = nodes[noff[g] + 1:noff[g + 1]]
        if seq in gts:
            emit(report_line(seq, 'optimized', absolute_trajectory_error(traj, gts[seq])))
        names = [graphs[seq][5][int(e)] for e in np.nonzero(pruned[eoff[g]:eoff[g + 1]])[0]]
        emit(f'seq {seq} pose graph: {noff[g + 1] - noff[g]} nodes, {eoff[g + 1] - eoff[g]} edges, cost {res.initial_cost[g]:.6g} -> '
             f'{res.final_cost[g]:.6g}, {res.iterations[g]} iterations ({res.stop_reasons[g]}), pruned edges: {names}')
        if covariance:
            cov = uncertainty(graphs[seq], nodes[noff[g]:noff[g + 1]], res.weights[int(eoff[g]):int(eoff[g + 1])].cpu().numpy(),
                              pruned[eoff[g]:eoff[g + 1]])
            emit(uncertainty_line(seq, cov))
            if args.out and not isinstance(cov, int):
                np.savetxt(osp.join(args.out, f'{seq}_optimized_covariance.txt'), cov.reshape(-1, 36), fmt='%.9e')
        if args.out:
            write_kitti_poses(osp.join(args.out, f'{seq}_optimized.txt'), nodes[noff[g]:noff[g + 1]])
        if scans:
            write_map(args, seq, 'optimized', scans[seq], nodes[noff[g]:noff[g + 1]], emit, to_prior=to_prior(seq)[0])
            if align:
                emit(to_prior(seq)[1])
        if getattr(args, 'map_refine', False):
            refine(seq, nodes[noff[g]:noff[g + 1]])
        if getattr(args, 'map_localize', False):
            localize(seq, nodes[noff[g]:noff[g + 1]])
    return res


def positive_finite(text):
    """argparse type: a float > 0 and finite."""
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f'{text!r} is not a number')
    if not (value > 0 and math.isfinite(value)):
        raise argparse.ArgumentTypeError(f'{text!r} is not positive and finite')
    return value


def make_parser():
    ap = argparse.ArgumentParser(prog='python -m rdmnet_amd.trajectory', description=__doc__.split('\n\n')[0])
    ap.add_argument('--features-root', '--features_root', required=True, help='directory of the {seq}_{src}_{ref}.npz pair files')
    ap.add_argument('--optimize', action='store_true', help='optimise the pose graphs of all sequences on the GPU')
    ap.add_argument('--line-process-weight', type=float, default=None, help='mu of the line process on the loop edges (default: none)')
    ap.add_argument('--edge-prune-threshold', type=float, default=0.25)
    ap.add_argument('--max-iterations', type=int, default=100)
    ap.add_argument('--unit-information', action='store_true', help='use the identity as the information matrix of every pair (the files need no `information`)')
    ap.add_argument('--preconditioner', choices=('block_jacobi', 'chain'), default='block_jacobi',
                    help='of the conjugate gradients inside --optimize: the node blocks, or the odometry chain factored exactly')
    ap.add_argument('--linear-solver', choices=('pcg', 'direct'), default='pcg',
                    help='of --optimize: conjugate gradients, or the direct sparse solve for a chain with loop closures')
    ap.add_argument('--covariance', action='store_true',
                    help='after --optimize: the marginal covariance of every optimised pose given frame 0 -- an `optimized uncertainty:` '
                         'line per sequence and, with --out, {seq}_optimized_covariance.txt (one 6 x 6 block per frame, rotation first)')
    ap.add_argument('--loop-consistency', action='store_true',
                    help='per sequence, the squared Mahalanobis distance d2 of every loop edge from the relative pose the odometry chain '
                         'gives, under the chain\'s uncertainty plus the edge\'s own (GPU; works without --optimize): a `loop consistency:` '
                         'line and, with --out, {seq}_loop_consistency.txt (file, s, t, d2 per loop edge).  d2 is only as calibrated as '
                         'the information matrices are: Open3D\'s scales with the number of correspondences, so it is no chi-square value')
    ap.add_argument('--loop-gate', type=positive_finite, default=None, metavar='D2',
                    help='with --optimize (implies --loop-consistency; no default): loop edges with d2 > D2 are left out of the optimised '
                         'graph.  The threshold is yours to choose from the d2 of your runs, not a chi-square quantile (see above)')
    ap.add_argument('--out', default=None, help='directory for one KITTI-format pose file per sequence and variant')
    ap.add_argument('--map-scans', default=None, metavar='DATASET_ROOT',
                    help='fuse the scans of every chain frame under each trajectory into a voxel map on the GPU, written to --out as '
                         '{seq}_{variant}_map.npy (float32 [M, C + 1]: the per-voxel means, then the count); reads '
                         'DATASET_ROOT/downsampled_xyzi/%%02d/%%06d.npy')
    ap.add_argument('--map-raw', action='store_true', help='read DATASET_ROOT/sequences/%%02d/velodyne/%%06d.bin instead')
    ap.add_argument('--map-voxel', type=float, default=MAP_DEFAULTS['voxel'], help='voxel edge in metres')
    ap.add_argument('--map-min-points', type=int, default=MAP_DEFAULTS['min_points'], help='write the voxels with at least this many points')
    ap.add_argument('--map-range', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                    help='integrate the points whose range in the sensor frame is within [LO, HI] metres (default: all)')
    ap.add_argument('--map-batch', type=int, default=MAP_DEFAULTS['batch'], help='scans per host-to-device copy and integrate call')
    ap.add_argument('--map-sharpness', action='store_true',
                    help='keep per-voxel second moments and print, after every map line, the mean plane thickness and the mean map '
                         'entropy of that map (needs --map-scans); lower is sharper')
    ap.add_argument('--map-sharpness-min-points', type=int, default=MAP_DEFAULTS['sharpness_min_points'], metavar='N',
                    help='take the sharpness report over the voxels with at least N >= 2 points')
    ap.add_argument('--map-min-scans', type=int, default=MAP_DEFAULTS['min_scans'], metavar='N',
                    help='keep only the voxels seen in at least N scans in every map that is written or reported (needs --map-scans): '
                         'removes what was in a voxel in fewer scans, such as a moving object; a `persistent:` line says what was kept')
    ap.add_argument('--map-refine', action='store_true',
                    help='register every frame against the voxel map of the frames before it and fuse it under the result: a third '
                         'variant, `refined`, from the optimised poses with --optimize, else the chained (needs --map-scans and --out)')
    ap.add_argument('--map-refine-sigma', type=float, default=REFINE_DEFAULTS['sigma'], metavar='S',
                    help='the noise of a scan point in metres, added to every voxel covariance')
    ap.add_argument('--map-refine-neighbors', type=int, choices=(1, 7), default=REFINE_DEFAULTS['neighbors'],
                    help="a point is matched to its own voxel (1) or to it and its six face neighbours (7: a wider basin)")
    ap.add_argument('--map-refine-iterations', type=int, default=REFINE_DEFAULTS['iterations'], metavar='N',
                    help='at most N Gauss-Newton updates per frame')
    ap.add_argument('--map-refine-robust', type=positive_finite, default=None, metavar='MU',
                    help='weight every point-voxel pair of --map-refine and --map-localize by (MU / (MU + d2))^2, d2 its squared '
                         'Mahalanobis distance, so that what stands elsewhere in a scan than in the map does not pull the pose; 9 is a '
                         'value to start from (default: off, every pair has weight one)')
    ap.add_argument('--map-refine-min-scans', type=int, default=REFINE_DEFAULTS['min_scans'], metavar='N',
                    help='register frame k >= N against the voxels seen in at least N of the frames before it (needs --map-refine)')
    ap.add_argument('--map-clean', action='store_true',
                    help="judge every point of every scan by each variant's full map and write the scans without what is not static "
                         'to --out as {seq}_{variant}_clean/ (needs --map-scans, --out and --map-min-scans N >= 2 or '
                         '--map-clean-max-d2 D); a `clean:` line says what was dropped')
    ap.add_argument('--map-clean-max-d2', type=float, default=CLEAN_DEFAULTS['max_d2'], metavar='D',
                    help="drop a point whose squared Mahalanobis distance from its voxel's Gaussian exceeds D (the map then keeps "
                         'second moments; default: no test)')
    ap.add_argument('--map-clean-sigma', type=float, default=CLEAN_DEFAULTS['sigma'], metavar='S',
                    help='the noise of a scan point in metres, added to every voxel covariance')
    ap.add_argument('--map-clean-neighbors', type=int, choices=(1, 7), default=CLEAN_DEFAULTS['neighbors'],
                    help='a point is judged by its own voxel (1) or by the best of it and its six face neighbours (7)')
    ap.add_argument('--map-save', action='store_true',
                    help="also write every variant's full map, before the --map-min-scans prune, to --out as {seq}_{variant}_map_state.npz: "
                         'the integers the map consists of, from which it reloads bit for bit (needs --map-scans)')
    ap.add_argument('--map-prior', default=None, metavar='FILE',
                    help='a saved map state in the world frame of the trajectory, such as an earlier --map-save of the same sequence: with '
                         '--map-clean the scans are judged by it instead of by their own map (--map-min-scans then counts its scans)')
    ap.add_argument('--map-localize', action='store_true',
                    help='register every frame, independently, against the fixed --map-prior (which needs moments): a variant `localized`, '
                         'from the optimised poses with --optimize, else the chained; --map-batch frames per call, sigma, neighbours and '
                         'iterations from the --map-refine-* options (needs --map-prior, --map-scans and --out)')
    ap.add_argument('--map-prior-align', action='store_true',
                    help="the --map-prior may live in any frame: align the base variant's map (optimised with --optimize, else chained, "
                         'with moments at --map-voxel) to it on the voxel Gaussians of both, write the transform T (prior <- trajectory) as '
                         '{seq}_prior_alignment.txt and ask the prior about T pose; sigma, neighbours and iterations from the '
                         '--map-refine-* options (needs --map-prior with moments, --map-scans and --out)')
    ap.add_argument('--map-prior-initial', default=None, metavar='FILE',
                    help='where --map-prior-align starts: a text file of 12 or 16 numbers, row-major, prior <- trajectory (default: the '
                         'identity); the basin is about one voxel of the prior with --map-refine-neighbors 7')
    return ap


def main(argv=None):
    args = make_parser().parse_args(argv)
    if not osp.isdir(args.features_root):
        sys.exit(f'{args.features_root}: not a directory')
    try:
        run(args)
    except TrajectoryError as e:
        sys.exit(str(e))


if __name__ == '__main__':
    main()
