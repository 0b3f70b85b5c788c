"""Times the voxel map (ops.VoxelMap) on synthetic scans along a synthetic drive.

  python tools/map_bench.py [--frames 256] [--points 120000 | 18000] [--reps 3] [--batch 64] [--voxel 0.3] [--cpu] [--cpu-frames 8]
                              [--moments] [--observations] [--register [--robust MU]] [--align] [--query] [--merge] [--digest]
With --digest (and nothing else): no timing, one sha1 line per output of the voxel map on the bundled scans (see digest()), for
comparing the bits of two builds of the library.  Otherwise prints one JSON line per case:
  * integrate: --frames scans of --points points (120 000: a raw scan; 18 000: a down-sampled one), xyz + intensity, integrated in
    batches of --batch from device memory into a table created large enough (no growth inside the timing); device time between
    two events, median of --reps; points/s, the bytes/s of integer atomic adds that implies ((8 C + 4) B a point: C int64 sums and
    a uint32 count), that rate as a fraction of the 1.3 TB/s the chip sustains for fp32 atomic adds, and the bytes/s of points read;
  * host copy: one batch from pageable and from pinned host memory to the device, points/s -- what the command line, which reads
    its scans from disk through host memory, is bound by at the latest;
  * extract: ms for the voxels of that map (select, radix sort of the slots, emit), and the voxels per second;
  * rehash: ms for one rdm_voxel_map_rehash of that map into a table of twice the capacity;
  * with --moments: the same integrate into a map with the nine second-moment sums beside it (ops.VoxelMap(moments=True): 14 integer
    atomic adds a point instead of 5, (8 C + 4 + 72) B), its points/s and the ratio to the plain integrate of the same run, and
    the ms of extract_moments (select, sort, covariance and the Jacobi eigen-solver per voxel);
  * with --observations: the same integrate into a map with the observations block beside it (ops.VoxelMap(observations=True): per
    point one load of the slot's mask more and, on a voxel's first sighting of a scan, four integer atomics), its points/s and the
    ratio to the plain integrate of the same run; the ms of extract_observations and of one pruned(2); and what --map-refine-min-scans 2
    adds to a frame of the refinement: one scan registered against a map with moments and observations of min(--frames, 64) scans
    at the command line's capacity, and against its pruned(2), the prune included;
  * with --register (and nothing else of the above): the scan-to-map registration (ops.VoxelMap.register) at neighbors 1 and 7 for both
    scan shapes (120 000 and 18 000 points), against the map with moments of min(--frames, 64) scans, from poses 5 cm / 5 mrad off: ms
    per evaluation (max_iteration = 0, one scan), ms per full registration of one scan and of a batch of 64 scans (default
    tolerances), the point-voxel pairs per second of the evaluation, and ms per iteration (accumulate + finalize launches) from runs
    of 4 and 12 forced updates of the batch; with --cpu also the seconds of one evaluation by tests/voxel_register_restatement.py
    and whether its counts equal the GPU's; with --robust MU also ms per evaluation and per registration of one scan with the robust
    weights (robust_scale MU) beside the plain form's, and ms per iteration of the batch of 64 likewise, the two alternated call by
    call in one process (`*_alternated`: the plain form's figures of that alternation), their ratios, and the scan's correspondences
    by weight;
  * with --align (and nothing else of the above): the map-to-map alignment (ops.VoxelMap.align) at neighbors 1 and 7 for both scan
    shapes: the target is --register's map of min(--frames, 64) scans, the source the map with moments of the same scans built in a
    frame turned by 0.3 rad and shifted by 3 m, the start 5 cm / 5 mrad off the transform between the two: ms per evaluation
    (max_iteration = 0), the record-voxel pairs per second of the evaluation, ms per full alignment (default tolerances) and ms per
    iteration from runs of 4 and 12 forced updates; beside them, from the same run and against the same target, ms per evaluation
    and pairs per second of --register's one scan; with --cpu also the seconds of one evaluation by
    tests/voxel_align_restatement.py on maps of the first --cpu-frames scans and whether its counts equal the GPU's;
  * with --query (and nothing else of the above): the per-point queries (ops.VoxelMap.query) for both scan shapes, a batch of
    min(--frames, 64) scans under their true poses against the map with moments and observations that holds them: points/s of a
    labels-only query that is the lookup alone (neighbors 1, min_scans 1), with the scan count (min_scans 2), with the distance too
    (max_d2 25) and at neighbors 7, and of a query with every output at neighbors 1 and 7; beside them the points/s of
    rdm_voxel_map_integrate of the same batch into a plain map that already holds it, and of rdm_voxel_map_integrate_observed into the
    queried map -- the same lookup plus the atomic adds --, both through the raw calls (no growth, no read-back); every figure is
    the whole call between two device events (a query: the kernel, the zeroing of the tallies and the upload of poses and offsets),
    ten calls a window; with --cpu also the
    seconds of tests/voxel_query_restatement.py on the first --cpu-frames scans and whether the GPU's integer outputs equal it;
  * with --merge (and nothing else of the above): the state calls behind save, load and merge on a map with moments and observations of
    min(--frames, 64) scans: ms and records/s of rdm_voxel_map_export (select, sort, emit of the raw integers), ms and records/s of
    rdm_voxel_map_import of those records into an empty map of the same capacity (C + 13 integer atomics a record; the reset before
    it is timed alone and taken out), and beside them the rehash of the same map with both blocks into a table of the same capacity,
    which moves the same slots with plain stores;
  * with --cpu: the NumPy restatement (tests/voxel_map_restatement.py) on the first --cpu-frames scans, its points/s, and whether the
    GPU's map of the same scans equals it bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

FLOAT_ATOMIC_BYTES_PER_S = 1.3e12  # the chip-wide rate of fp32 atomic adds


def timed(fn, reps):
    """Median device time in ms of fn() between two events, after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def timed_alternated(fn_a, fn_b, reps):
    """Median device times in ms of fn_a() and fn_b(), called in turn (a, b, a, b, ...) after one warm-up call of each
    -> (ms_a, ms_b, the last output of fn_a, of fn_b)."""
    import torch
    fn_a()
    fn_b()
    torch.cuda.synchronize()
    times, out = ([], []), [None, None]
    for _ in range(reps):
        for k, fn in enumerate((fn_a, fn_b)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return float(np.median(times[0])), float(np.median(times[1])), out[0], out[1]


def synthetic_scans(frames, points, seed=0):
    """-> float32 CUDA [frames * points, 4] in the sensor frame: a ground plane at z = -1.7 m with structures up to 4 m on 30 % of
    the points, denser near the sensor (r = 2 + 78 u^2 m), intensity in [0, 1).  Generated on the device."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    n = frames * points
    u = torch.rand((n, 5), generator=g, device='cuda')
    r = 2.0 + 78.0 * u[:, 0] ** 2
    th = 2.0 * np.pi * u[:, 1]
    z = -1.7 + 0.05 * (u[:, 2] - 0.5) + (u[:, 3] < 0.3) * 4.0 * u[:, 2]
    return torch.stack([r * torch.cos(th), r * torch.sin(th), z, u[:, 4]], 1).contiguous()


def drive(frames, step=1.0):
    """One pose per frame: `step` metres forward per frame along a heading that turns slowly, with a little roll."""
    poses = np.zeros((frames, 4, 4))
    x = y = 0.0
    for k in range(frames):
        yaw = 0.6 * np.sin(k / 80.0)
        roll = 0.01 * np.sin(k / 7.0)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
        poses[k, :3, :3] = Rz @ Rx
        poses[k, :3, 3] = [x, y, 0.02 * k]
        poses[k, 3, 3] = 1.0
        x += step * np.cos(yaw)
        y += step * np.sin(yaw)
    return poses


def off_poses(poses, rng):
    """The poses 5 mrad / 5 cm (one sigma per axis) off."""
    off = poses.copy()
    for X in off:
        w = rng.normal(0.0, 0.005, 3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        X[:3, :3] = (np.eye(3) + K + 0.5 * K @ K) @ X[:3, :3]
        X[:3, 3] += rng.normal(0.0, 0.05, 3)
    return off


def digest():
    """One `sha1  what` line over the raw bytes of everything the voxel map returns for the three bundled scans (tests/golden/scans.npz
    with the intensity column of the tests) under three seeded poses: stats, extract and extract_moments of maps that grow from 1024
    slots at voxel 0.3 and 0.05, with and without moments, and every field of register at neighbors 1 and 7, as one batch of three
    and as three calls of one; then the same registrations with robust_scale = 9, align of a map of voxel 0.5 onto the map of voxel
    0.3, query with every output on a map with moments and observations grown scan by scan from 64 slots, that map's
    extract_observations, the state of its pruned(min_scans=2), its own state, and the state of two halves merged.  Two libraries
    (RDM_LIB_PATH) compute the same bits iff they print the same lines."""
    import hashlib
    import torch
    from rdmnet_amd import ops
    from test_voxel_map import random_pose, with_attribute
    scans = np.load(os.path.join(ROOT, 'tests', 'golden', 'scans.npz'))
    clouds = [torch.from_numpy(with_attribute(scans[k], i)).cuda() for i, k in enumerate(('s000000', 's000004', 's000007'))]
    rng = np.random.default_rng(11)
    poses = np.stack([random_pose(rng) for _ in clouds])

    def line(what, tensors):
        h = hashlib.sha1()
        for t in tensors:
            h.update(t.cpu().contiguous().numpy().tobytes())
        print(f'{h.hexdigest()}  {what}', flush=True)

    for voxel in (0.3, 0.05):
        for moments in (True, False):
            vmap = ops.VoxelMap(voxel, channels=4, capacity=1024, moments=moments).integrate(clouds, poses)
            name = f'voxel {voxel} moments {int(moments)}'
            line(f'{name} stats', [torch.tensor(list(vmap.stats().values()), dtype=torch.int64)])
            line(f'{name} extract', vmap.extract())
            if moments:
                line(f'{name} extract_moments', vmap.extract_moments())
    vmap = ops.VoxelMap(0.3, channels=4, capacity=1024, moments=True).integrate(clouds, poses)
    off = off_poses(poses, np.random.default_rng(0))
    for neighbors in (1, 7):
        runs = [vmap.register(clouds, off, neighbors=neighbors, max_iteration=5)]
        runs += [vmap.register(clouds[k:k + 1], off[k:k + 1], neighbors=neighbors, max_iteration=5) for k in range(3)]
        for what, res in zip(('batch of 3', 'scan 0', 'scan 1', 'scan 2'), runs):
            line(f'register neighbors {neighbors} {what}', [res.transformations, res.information, res.gradient, res.cost, res.iterations,
                                                            res.num_correspondences, res.num_points, res.status])

    def fields(res):
        return [res.transformations, res.information, res.gradient, res.cost, res.iterations, res.num_correspondences, res.num_points,
                res.status] + ([] if res.weight_sum is None else [res.weight_sum])

    def state_line(what, st):
        host = torch.tensor(list(st['counters'].values()) + [st['num_scans']], dtype=torch.int64)
        line(what, [st[k] for k in ('keys', 'counts', 'sums', 'moments', 'observations') if k in st] + [host])

    for neighbors in (1, 7):
        kw = dict(neighbors=neighbors, max_iteration=5, robust_scale=9)
        runs = [vmap.register(clouds, off, **kw)] + [vmap.register(clouds[k:k + 1], off[k:k + 1], **kw) for k in range(3)]
        for what, res in zip(('batch of 3', 'scan 0', 'scan 1', 'scan 2'), runs):
            line(f'register robust 9 neighbors {neighbors} {what}', fields(res))
    source = ops.VoxelMap(0.5, channels=4, capacity=1024, moments=True).integrate(clouds, poses)
    start = off_poses(np.eye(4)[None], np.random.default_rng(1))
    for neighbors in (1, 7):  # (the bundled scans are sparse: two points make a voxel here, or hardly a pair is left)
        kw = dict(neighbors=neighbors, max_iteration=5, min_points=2, source_min_points=2)
        line(f'align voxel 0.5 onto 0.3 neighbors {neighbors}', fields(vmap.align([source], start, **kw)))
    full = ops.VoxelMap(0.3, channels=4, capacity=64, moments=True, observations=True)
    for k in range(3):
        full.integrate(clouds[k:k + 1], poses[k:k + 1])
    for neighbors in (1, 7):
        res = full.query(clouds, off, neighbors=neighbors, min_scans=2, max_d2=25.0)
        line(f'query every output neighbors {neighbors}', [getattr(res, k) for k in res.FIELDS])
    line('extract_observations', full.extract_observations())
    state_line('pruned(min_scans=2) state', full.pruned(min_scans=2).state())
    state_line('state of a map grown from 64 slots', full.state())
    halves = [ops.VoxelMap(0.3, channels=4, capacity=1024, moments=True, observations=True).integrate(clouds[a:b], poses[a:b])
              for a, b in ((0, 2), (2, 3))]
    state_line('merge of two halves state', halves[0].merge(halves[1]).state())
    return 0


def register_cases(a):
    import torch
    from rdmnet_amd import ops
    rng = np.random.default_rng(0)
    frames = max(min(a.frames, 64), 1)
    for points in (120000, 18000):
        cloud, poses = synthetic_scans(frames, points), drive(frames)
        clouds = [cloud[k * points:(k + 1) * points] for k in range(frames)]
        vmap = ops.VoxelMap(a.voxel, channels=4, capacity=1 << 24, moments=True).integrate(clouds, poses)
        off = off_poses(poses, rng)
        batch = [clouds[k % frames] for k in range(64)]
        Xb = np.stack([off[k % frames] for k in range(64)])
        for neighbors in (1, 7):
            kw = dict(neighbors=neighbors)
            ms_eval, ev = timed(lambda: vmap.register(clouds[:1], off[:1], max_iteration=0, **kw), a.reps)
            ms_one, one = timed(lambda: vmap.register(clouds[:1], off[:1], **kw), a.reps)
            ms_batch, many = timed(lambda: vmap.register(batch, Xb, **kw), a.reps)
            ms_4, _ = timed(lambda: vmap.register(batch, Xb, max_iteration=4, rot_eps=0.0, trans_eps=0.0, **kw), a.reps)
            ms_12, _ = timed(lambda: vmap.register(batch, Xb, max_iteration=12, rot_eps=0.0, trans_eps=0.0, **kw), a.reps)
            pairs = int(ev.num_correspondences[0])
            line = {'case': 'register', 'points_per_scan': points, 'neighbors': neighbors, 'voxel': a.voxel, 'map_frames': frames,
                    'voxels': len(vmap), 'ms_per_evaluation': round(ms_eval, 3), 'pairs_per_evaluation': pairs,
                    'pairs_per_s': round(pairs / ms_eval * 1e3), 'ms_one_scan': round(ms_one, 3), 'iterations_one_scan': int(one.iterations[0]),
                    'status_one_scan': int(one.status[0]), 'ms_batch_of_64': round(ms_batch, 3),
                    'mean_iterations_batch': round(float(many.iterations.double().mean()), 2),
                    'converged_in_batch': int((many.status == 1).sum()),
                    'ms_per_iteration_batch_of_64': round((ms_12 - ms_4) / 8.0, 4),
                    'pairs_per_s_batch': round(float(many.num_correspondences.sum()) / ((ms_12 - ms_4) / 8.0) * 1e3)}
            if a.robust is not None:
                rkw = dict(kw, robust_scale=a.robust)
                ev_p, ev_w, _, wev = timed_alternated(lambda: vmap.register(clouds[:1], off[:1], max_iteration=0, **kw),
                                                      lambda: vmap.register(clouds[:1], off[:1], max_iteration=0, **rkw), a.reps)
                one_p, one_w, _, wone = timed_alternated(lambda: vmap.register(clouds[:1], off[:1], **kw),
                                                         lambda: vmap.register(clouds[:1], off[:1], **rkw), a.reps)
                forced = dict(rot_eps=0.0, trans_eps=0.0)
                p4, w4, _, _ = timed_alternated(lambda: vmap.register(batch, Xb, max_iteration=4, **forced, **kw),
                                                lambda: vmap.register(batch, Xb, max_iteration=4, **forced, **rkw), a.reps)
                p12, w12, _, _ = timed_alternated(lambda: vmap.register(batch, Xb, max_iteration=12, **forced, **kw),
                                                  lambda: vmap.register(batch, Xb, max_iteration=12, **forced, **rkw), a.reps)
                line.update(ms_per_iteration_batch_of_64_alternated=round((p12 - p4) / 8.0, 4),
                            ms_per_iteration_batch_of_64_weighted=round((w12 - w4) / 8.0, 4),
                            weighted_over_plain_iteration_batch=round((w12 - w4) / (p12 - p4), 3))
                line.update(robust_scale=a.robust, ms_per_evaluation_alternated=round(ev_p, 3), ms_per_evaluation_weighted=round(ev_w, 3),
                            weighted_over_plain_evaluation=round(ev_w / ev_p, 3), ms_one_scan_alternated=round(one_p, 3),
                            ms_one_scan_weighted=round(one_w, 3), weighted_over_plain_one_scan=round(one_w / one_p, 3),
                            iterations_one_scan_weighted=int(wone.iterations[0]), status_one_scan_weighted=int(wone.status[0]),
                            weight_sum_per_evaluation=round(float(wev.weight_sum[0]), 1))
            if a.cpu:
                import voxel_moments_restatement as MR
                import voxel_register_restatement as RR
                m = min(a.cpu_frames, frames)
                table = MR.build([c.cpu().numpy() for c in clouds[:m]], poses[:m], a.voxel, 4)
                small = ops.VoxelMap(a.voxel, channels=4, moments=True).integrate(clouds[:m], poses[:m])
                got = small.register(clouds[:1], off[:1], max_iteration=0, **kw)
                t0 = time.perf_counter()
                e = RR.evaluate(table, clouds[0].cpu().numpy(), off[0], 0.02, 4, neighbors)
                line.update(cpu_s_per_evaluation=round(time.perf_counter() - t0, 4), cpu_map_frames=m,
                            counts_equal=bool(int(got.num_correspondences[0]) == e['n_corr'] and int(got.num_points[0]) == e['n_points']))
            print(json.dumps(line), flush=True)
        del vmap
    return 0


def align_cases(a):
    from rdmnet_amd import ops
    rng = np.random.default_rng(0)
    frames = max(min(a.frames, 64), 1)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [2.5, -1.5, 0.4]
    start = off_poses(T[None], rng)
    for points in (120000, 18000):
        cloud, poses = synthetic_scans(frames, points), drive(frames)
        clouds = [cloud[k * points:(k + 1) * points] for k in range(frames)]
        vmap = ops.VoxelMap(a.voxel, channels=4, capacity=1 << 24, moments=True).integrate(clouds, poses)
        moved = np.linalg.inv(T) @ poses
        source = ops.VoxelMap(a.voxel, channels=4, capacity=1 << 24, moments=True).integrate(clouds, moved)
        state = source.state()  # exported once: the timings are the alignment's own
        off = off_poses(poses, rng)
        for neighbors in (1, 7):
            kw = dict(neighbors=neighbors)
            ms_eval, ev = timed(lambda: vmap.align([state], start, max_iteration=0, **kw), a.reps)
            ms_one, one = timed(lambda: vmap.align([state], start, **kw), a.reps)
            ms_4, _ = timed(lambda: vmap.align([state], start, max_iteration=4, rot_eps=0.0, trans_eps=0.0, **kw), a.reps)
            ms_12, _ = timed(lambda: vmap.align([state], start, max_iteration=12, rot_eps=0.0, trans_eps=0.0, **kw), a.reps)
            ms_reg, reg = timed(lambda: vmap.register(clouds[:1], off[:1], max_iteration=0, **kw), a.reps)
            pairs, reg_pairs = int(ev.num_correspondences[0]), int(reg.num_correspondences[0])
            line = {'case': 'align', 'points_per_scan': points, 'neighbors': neighbors, 'voxel': a.voxel, 'map_frames': frames,
                    'target_voxels': len(vmap), 'source_voxels': len(source), 'source_records_passed': int(ev.num_points[0]),
                    'ms_per_evaluation': round(ms_eval, 3), 'pairs_per_evaluation': pairs, 'pairs_per_s': round(pairs / ms_eval * 1e3),
                    'ms_per_alignment': round(ms_one, 3), 'iterations': int(one.iterations[0]), 'status': int(one.status[0]),
                    'ms_per_iteration': round((ms_12 - ms_4) / 8.0, 4), 'register_ms_per_evaluation': round(ms_reg, 3),
                    'register_pairs_per_evaluation': reg_pairs, 'register_pairs_per_s': round(reg_pairs / ms_reg * 1e3)}
            if a.cpu:
                import voxel_align_restatement as AR
                import voxel_moments_restatement as MR
                m = min(a.cpu_frames, frames)
                host = [c.cpu().numpy() for c in clouds[:m]]
                target, src = MR.build(host, poses[:m], a.voxel, 4), MR.build(host, moved[:m], a.voxel, 4)
                small = ops.VoxelMap(a.voxel, channels=4, moments=True).integrate(clouds[:m], poses[:m])
                small_src = ops.VoxelMap(a.voxel, channels=4, moments=True).integrate(clouds[:m], moved[:m])
                got = small.align([small_src], start, max_iteration=0, **kw)
                t0 = time.perf_counter()
                e = AR.evaluate(target, src, start[0], 0.02, 4, 4, neighbors)
                line.update(cpu_s_per_evaluation=round(time.perf_counter() - t0, 4), cpu_map_frames=m,
                            counts_equal=bool(int(got.num_correspondences[0]) == e['n_corr'] and int(got.num_points[0]) == e['n_points']))
            print(json.dumps(line), flush=True)
        del vmap, source, state
    return 0


def query_cases(a):
    import torch
    from rdmnet_amd import _lib, ops
    L = _lib.lib()
    frames = max(min(a.frames, 64), 1)
    for points in (120000, 18000):
        cloud, poses = synthetic_scans(frames, points), drive(frames)
        total = frames * points
        clouds = [cloud[k * points:(k + 1) * points] for k in range(frames)]
        packed = (cloud, (torch.arange(frames + 1, dtype=torch.int64) * points).cuda())
        capacity = 1 << int(np.ceil(np.log2(4 * total)))  # no growth in any of the calls below
        vmap = ops.VoxelMap(a.voxel, channels=4, capacity=capacity, moments=True, observations=True).integrate(packed, poses)
        plain = ops.VoxelMap(a.voxel, channels=4, capacity=capacity).integrate(packed, poses)
        assert vmap.capacity == plain.capacity == capacity
        X = torch.from_numpy(poses).cuda()
        batch = (cloud.data_ptr(), 4, total, packed[1].data_ptr(), X.data_ptr(), frames, 0.0, float('inf'))

        def integrate_plain():
            _lib.check(L.rdm_voxel_map_integrate(*plain._head(), a.voxel, *batch, _lib.stream_ptr()), 'integrate')

        def integrate_full():
            _lib.check(L.rdm_voxel_map_integrate_observed(*vmap._head(), a.voxel, *batch, vmap._mom.data_ptr(), vmap._mom.numel(),
                                                          vmap._obs.data_ptr(), vmap._obs.numel(), frames, _lib.stream_ptr()), 'integrate_observed')

        line = {'case': 'query', 'points_per_scan': points, 'scans': frames, 'points': total, 'voxel': a.voxel, 'capacity': capacity,
                'voxels': len(vmap)}
        inner = 10  # calls per timed window: one call of 18 000-point scans is a fraction of a millisecond
        line['calls_per_window'] = inner
        ms_plain = timed(lambda: [integrate_plain() for _ in range(inner)], a.reps)[0] / inner
        line['integrate_plain_points_per_s'] = round(total / ms_plain * 1e3)
        cases = (('labels_lookup_only_n1', dict(outputs=('labels',), neighbors=1, min_scans=1)),
                 ('labels_min_scans_n1', dict(outputs=('labels',), neighbors=1, min_scans=2)),
                 ('labels_min_scans_max_d2_n1', dict(outputs=('labels',), neighbors=1, min_scans=2, max_d2=25.0)),
                 ('labels_min_scans_n7', dict(outputs=('labels',), neighbors=7, min_scans=2)),
                 ('labels_tallies_min_scans_n1', dict(outputs=('labels', 'tallies'), neighbors=1, min_scans=2)),
                 ('every_output_n1', dict(neighbors=1, min_scans=2, max_d2=25.0)),
                 ('every_output_n7', dict(neighbors=7, min_scans=2, max_d2=25.0)))
        for name, kw in cases:
            ms, res = timed(lambda: [vmap.query(packed, poses, **kw) for _ in range(inner)][-1], a.reps)
            ms /= inner
            line[name + '_points_per_s'] = round(total / ms * 1e3)
            line[name + '_over_integrate_plain'] = round(ms_plain / ms, 3)
        line['tallies'] = res.tallies.sum(0).tolist()
        ms_full = timed(lambda: [integrate_full() for _ in range(inner)], a.reps)[0] / inner  # (last: it adds to the queried map)
        line['integrate_moments_observations_points_per_s'] = round(total / ms_full * 1e3)
        if a.cpu:
            import voxel_moments_restatement as MR
            import voxel_observations_restatement as OR
            import voxel_query_restatement as QR
            m = min(a.cpu_frames, frames)
            host = [c.cpu().numpy() for c in clouds[:m]]
            table, observed = MR.build(host, poses[:m], a.voxel, 4), OR.build(host, poses[:m], a.voxel, 4)
            small = ops.VoxelMap(a.voxel, channels=4, moments=True, observations=True).integrate(clouds[:m], poses[:m])
            got = small.query(clouds[:m], poses[:m], neighbors=7, min_scans=2, max_d2=25.0)
            t0 = time.perf_counter()
            ref = QR.batch(table, observed, host, poses[:m], neighbors=7, min_scans=2, max_d2=25.0)
            cpu_s = time.perf_counter() - t0
            line.update(cpu_s=round(cpu_s, 3), cpu_frames=m, cpu_points_per_s=round(m * points / cpu_s),
                        integers_equal=bool(all(np.array_equal(getattr(got, k).cpu().numpy(), ref[k]) for k in QR.INTEGERS + ('tallies',))))
        print(json.dumps(line), flush=True)
        del vmap, plain
    return 0


def merge_cases(a):
    """--merge: the two state calls on a map with moments and observations of min(--frames, 64) scans, through the raw calls into
    preallocated arrays (no growth, no read-back inside the timing), and the rehash of the same map as the yardstick."""
    import torch
    from rdmnet_amd import _lib, ops
    L, C = _lib.lib(), 4
    frames = min(a.frames, 64)
    cloud, poses = synthetic_scans(frames, a.points), drive(frames)
    capacity = min(1 << max(int(np.ceil(np.log2(2 * frames * a.points))), 6), 1 << 28)
    vmap = ops.VoxelMap(a.voxel, channels=C, capacity=capacity, moments=True, observations=True)
    vmap.integrate((cloud, (torch.arange(frames + 1, dtype=torch.int64) * a.points).cuda()), poses)
    st = vmap.stats()
    rows = st['occupied']
    assert vmap.capacity == capacity and st['dropped_full'] == 0
    rec = dict(keys=torch.empty((rows,), dtype=torch.uint64, device='cuda'), counts=torch.empty((rows,), dtype=torch.uint32, device='cuda'),
               sums=torch.empty((rows, C), dtype=torch.int64, device='cuda'), moments=torch.empty((rows, 9), dtype=torch.int64, device='cuda'),
               seen=torch.empty((rows, 3), dtype=torch.int32, device='cuda'))
    n_rows = torch.zeros((1,), dtype=torch.int64, device='cuda')
    ws = torch.empty((L.rdm_voxel_map_extract_workspace_bytes(capacity),), dtype=torch.uint8, device='cuda')
    ptrs = [rec[k].data_ptr() for k in ('keys', 'counts', 'sums', 'moments', 'seen')]
    ms_export, _ = timed(lambda: _lib.check(L.rdm_voxel_map_export(*vmap._head(), *vmap._blocks(), 1, *ptrs, rows, n_rows.data_ptr(),
                                                                  ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'export'), a.reps)
    assert int(n_rows.item()) == rows
    record_bytes = 8 + 4 + 8 * C + 72 + 12
    print(json.dumps({'case': 'export', 'capacity': capacity, 'voxels': rows, 'ms': round(ms_export, 3),
                      'records_per_s': round(rows / ms_export * 1e3), 'bytes_per_record': record_bytes}))
    into = ops.VoxelMap(a.voxel, channels=C, capacity=capacity, moments=True, observations=True)
    n_rejected = torch.zeros((1,), dtype=torch.int64, device='cuda')

    def load():
        into.reset()
        _lib.check(L.rdm_voxel_map_import(*into._head(), *into._blocks(), *ptrs, rows, 0, 0, n_rejected.data_ptr(), _lib.stream_ptr()),
                   'import')

    ms_reset, _ = timed(into.reset, a.reps)
    ms_all, _ = timed(load, a.reps)
    ms_import = ms_all - ms_reset
    after = into.stats()
    assert int(n_rejected.item()) == 0 and (after['occupied'], after['integrated']) == (rows, st['integrated'])
    atomics = C + 13  # the count, C sums, nine moments, three observation fields
    print(json.dumps({'case': 'import', 'capacity': capacity, 'records': rows, 'ms': round(ms_import, 3), 'ms_reset_excluded': round(ms_reset, 3),
                      'records_per_s': round(rows / ms_import * 1e3), 'atomics_per_record': atomics,
                      'atomic_bytes_per_s': round(rows / ms_import * 1e3 * (record_bytes - 8))}))
    new, mom, obs = into._buf, into._mom, into._obs
    old = (vmap._buf.data_ptr(), vmap._buf.numel(), capacity)

    def rehash():
        _lib.check(L.rdm_voxel_map_rehash(*old, new.data_ptr(), new.numel(), capacity, C, _lib.stream_ptr()), 'rehash')
        _lib.check(L.rdm_voxel_moments_rehash(*old, vmap._mom.data_ptr(), vmap._mom.numel(), new.data_ptr(), new.numel(), capacity,
                                              mom.data_ptr(), mom.numel(), C, _lib.stream_ptr()), 'moments rehash')
        _lib.check(L.rdm_voxel_observations_rehash(*old, vmap._obs.data_ptr(), vmap._obs.numel(), new.data_ptr(), new.numel(), capacity,
                                                   obs.data_ptr(), obs.numel(), C, _lib.stream_ptr()), 'observations rehash')

    ms_rehash, _ = timed(rehash, a.reps)  # (its three resets are inside, as import's one reset is taken out: both move `rows` slots)
    print(json.dumps({'case': 'rehash with both blocks', 'capacity': capacity, 'voxels': rows, 'ms': round(ms_rehash, 3),
                      'ms_less_reset': round(ms_rehash - ms_reset, 3), 'import_over_rehash': round(ms_import / max(ms_rehash - ms_reset, 1e-6), 2)}))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--points', type=int, default=120000, help='points per scan: 120000 (raw) or 18000 (down-sampled)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64, help='scans per integrate call')
    ap.add_argument('--voxel', type=float, default=0.3)
    ap.add_argument('--moments', action='store_true', help='also time integrate and extract with the per-voxel second moments')
    ap.add_argument('--observations', action='store_true',
                    help='also time integrate with the per-voxel scan observations, extract_observations, pruned and a refinement frame')
    ap.add_argument('--register', action='store_true', help='time the scan-to-map registration and nothing else')
    ap.add_argument('--robust', type=float, default=None, metavar='MU',
                    help='with --register: also time the registration with robust weights of this scale, alternated with the plain form')
    ap.add_argument('--align', action='store_true', help='time the map-to-map alignment beside the registration and nothing else')
    ap.add_argument('--query', action='store_true', help='time the per-point queries beside integrate and nothing else')
    ap.add_argument('--merge', action='store_true', help='time the export and the import of a map state beside its rehash and nothing else')
    ap.add_argument('--digest', action='store_true', help='print the sha1 lines of the bundled scans\' maps and registrations and nothing else')
    ap.add_argument('--cpu', action='store_true', help='also time the NumPy restatement and compare the maps bit for bit')
    ap.add_argument('--cpu-frames', type=int, default=8)
    a = ap.parse_args(argv)
    if a.robust is not None and not (a.register and a.robust > 0 and np.isfinite(a.robust)):
        ap.error('--robust needs --register and a positive finite MU')
    import torch
    from rdmnet_amd import _lib, ops
    assert torch.cuda.is_available(), 'map_bench needs a GPU'
    if a.digest:
        return digest()
    if a.register:
        return register_cases(a)
    if a.align:
        return align_cases(a)
    if a.query:
        return query_cases(a)
    if a.merge:
        return merge_cases(a)
    C = 4
    cloud, poses = synthetic_scans(a.frames, a.points), drive(a.frames)
    total = a.frames * a.points
    capacity = 1 << max(int(np.ceil(np.log2(2 * total))), 6)  # what VoxelMap itself would grow to at the latest
    capacity = min(capacity, 1 << 28)
    vmap = ops.VoxelMap(a.voxel, channels=C, capacity=capacity)
    batches = []
    for lo in range(0, a.frames, a.batch):
        hi = min(lo + a.batch, a.frames)
        batches.append((cloud[lo * a.points:hi * a.points], (torch.arange(hi - lo + 1, dtype=torch.int64) * a.points).cuda(),
                        torch.from_numpy(poses[lo:hi])))

    def integrate():
        vmap.reset()
        for pts, off, X in batches:
            vmap.integrate((pts, off), X)
        return vmap

    def reset_only():
        vmap.reset()

    ms_reset, _ = timed(reset_only, a.reps)
    ms_all, _ = timed(integrate, a.reps)
    ms = ms_all - ms_reset
    st = vmap.stats()
    assert vmap.capacity == capacity and st['dropped_full'] == 0
    pps = total / ms * 1e3
    print(json.dumps({'case': 'integrate', 'frames': a.frames, 'points_per_scan': a.points, 'batch': a.batch, 'voxel': a.voxel,
                      'capacity': capacity, 'ms': round(ms, 3), 'ms_reset_excluded': round(ms_reset, 3), 'points_per_s': round(pps),
                      'atomic_bytes_per_s': round(pps * (8 * C + 4)),
                      'fraction_of_float_atomic_rate': round(pps * (8 * C + 4) / FLOAT_ATOMIC_BYTES_PER_S, 4),
                      'read_bytes_per_s': round(pps * 4 * C), 'voxels': st['occupied'],
                      'points_per_voxel': round(st['integrated'] / max(st['occupied'], 1), 2), 'stats': st}))

    if a.moments:
        mmap = ops.VoxelMap(a.voxel, channels=C, capacity=capacity, moments=True)

        def integrate_moments():
            mmap.reset()
            for pts, off, X in batches:
                mmap.integrate((pts, off), X)
            return mmap

        ms_mreset, _ = timed(mmap.reset, a.reps)
        ms_mall, _ = timed(integrate_moments, a.reps)
        ms_m = ms_mall - ms_mreset
        assert mmap.capacity == capacity and mmap.stats() == st
        pps_m = total / ms_m * 1e3
        print(json.dumps({'case': 'integrate with moments', 'ms': round(ms_m, 3), 'ms_reset_excluded': round(ms_mreset, 3),
                          'points_per_s': round(pps_m), 'over_plain_integrate': round(pps_m / pps, 3),
                          'atomic_bytes_per_s': round(pps_m * (8 * C + 4 + 72)),
                          'fraction_of_float_atomic_rate': round(pps_m * (8 * C + 4 + 72) / FLOAT_ATOMIC_BYTES_PER_S, 4)}))
        ms_xm, out_m = timed(lambda: mmap.extract_moments(), a.reps)
        print(json.dumps({'case': 'extract_moments', 'capacity': capacity, 'voxels': int(out_m[0].shape[0]), 'ms': round(ms_xm, 3),
                          'voxels_per_s': round(out_m[0].shape[0] / ms_xm * 1e3), 'sharpness': mmap.sharpness()}))
        del mmap, out_m

    if a.observations:
        omap = ops.VoxelMap(a.voxel, channels=C, capacity=capacity, observations=True)

        def integrate_observed():
            omap.reset()
            for pts, off, X in batches:
                omap.integrate((pts, off), X)
            return omap

        ms_oreset, _ = timed(omap.reset, a.reps)
        ms_oall, _ = timed(integrate_observed, a.reps)
        ms_o = ms_oall - ms_oreset
        assert omap.capacity == capacity and omap.stats() == st and omap.num_scans == a.frames
        pps_o = total / ms_o * 1e3
        print(json.dumps({'case': 'integrate with observations', 'ms': round(ms_o, 3), 'ms_reset_excluded': round(ms_oreset, 3),
                          'calls': sum(-(-(len(off) - 1) // _lib.VOXEL_OBSERVATIONS_MAX_SCANS) for _, off, _ in batches),
                          'points_per_s': round(pps_o), 'over_plain_integrate': round(pps_o / pps, 3)}))
        ms_xo, out_o = timed(lambda: omap.extract_observations(), a.reps)
        seen = torch.bincount(out_o[0].long()).cpu().tolist()
        print(json.dumps({'case': 'extract_observations', 'capacity': capacity, 'voxels': int(out_o[0].shape[0]), 'ms': round(ms_xo, 3),
                          'voxels_per_s': round(out_o[0].shape[0] / ms_xo * 1e3), 'voxels_seen_once': seen[1] if len(seen) > 1 else 0}))
        ms_p, kept = timed(lambda: omap.pruned(2), a.reps)
        print(json.dumps({'case': 'pruned', 'min_scans': 2, 'capacity': capacity, 'voxels': st['occupied'], 'kept': len(kept), 'ms': round(ms_p, 3)}))
        del omap, out_o, kept
        m = max(min(a.frames, 64), 1)
        rmap = ops.VoxelMap(a.voxel, channels=C, moments=True, observations=True)  # (the command line's capacity)
        rmap.integrate([cloud[k * a.points:(k + 1) * a.points] for k in range(m)], poses[:m])
        scan, X0 = [cloud[:a.points]], off_poses(poses[:1], np.random.default_rng(0))
        ms_full, r_full = timed(lambda: rmap.register(scan, X0), a.reps)
        ms_pruned, r_pruned = timed(lambda: rmap.pruned(2).register(scan, X0), a.reps)
        print(json.dumps({'case': 'refine frame', 'map_frames': m, 'capacity': rmap.capacity, 'ms_register_full_map': round(ms_full, 3),
                          'ms_prune_and_register': round(ms_pruned, 3), 'ms_added_by_min_scans_2': round(ms_pruned - ms_full, 3),
                          'iterations': [int(r_full.iterations[0]), int(r_pruned.iterations[0])],
                          'correspondences': [int(r_full.num_correspondences[0]), int(r_pruned.num_correspondences[0])]}))
        del rmap

    host = cloud[:min(a.batch, a.frames) * a.points].cpu().numpy()
    pinned = torch.from_numpy(host).pin_memory()
    for name, src in (('pageable', torch.from_numpy(host)), ('pinned', pinned)):
        t = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src.cuda()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        s = float(np.median(t[1:]))
        print(json.dumps({'case': 'host copy', 'memory': name, 'points': len(host), 'ms': round(s * 1e3, 3),
                          'points_per_s': round(len(host) / s), 'GB_per_s': round(host.nbytes / s / 1e9, 2),
                          'integrate_over_copy': round(pps / (len(host) / s), 2)}))

    ms_x, out = timed(lambda: vmap.extract(), a.reps)
    print(json.dumps({'case': 'extract', 'capacity': capacity, 'voxels': int(out[0].shape[0]), 'ms': round(ms_x, 3),
                      'voxels_per_s': round(out[0].shape[0] / ms_x * 1e3)}))

    L = _lib.lib()
    if L.rdm_voxel_map_bytes(2 * capacity, C):
        new = torch.empty((L.rdm_voxel_map_bytes(2 * capacity, C),), dtype=torch.uint8, device='cuda')
        ms_r, _ = timed(lambda: _lib.check(L.rdm_voxel_map_rehash(vmap._buf.data_ptr(), vmap._buf.numel(), capacity, new.data_ptr(),
                                                                  new.numel(), 2 * capacity, C, _lib.stream_ptr()), 'rehash'), a.reps)
        print(json.dumps({'case': 'rehash', 'from': capacity, 'to': 2 * capacity, 'voxels': st['occupied'], 'ms': round(ms_r, 3)}))
        del new

    if a.cpu:
        import voxel_map_restatement as VM
        m = min(a.cpu_frames, a.frames)
        clouds = [cloud[k * a.points:(k + 1) * a.points].cpu().numpy() for k in range(m)]
        t0 = time.perf_counter()
        ref = VM.build(clouds, poses[:m], a.voxel, C)
        want = ref.extract()
        cpu_s = time.perf_counter() - t0
        small = ops.VoxelMap(a.voxel, channels=C).integrate([cloud[k * a.points:(k + 1) * a.points] for k in range(m)], poses[:m])
        got = [t.cpu().numpy() for t in small.extract()]
        same = all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
                   for g, w in zip(got, want)) and small.stats() == ref.stats()
        print(json.dumps({'case': 'cpu restatement', 'frames': m, 'points': m * a.points, 'cpu_s': round(cpu_s, 3),
                          'cpu_points_per_s': round(m * a.points / cpu_s), 'gpu_points_per_s': round(pps),
                          'gpu_over_cpu': round(pps / (m * a.points / cpu_s), 1), 'voxels': len(want[0]), 'bit_equal': bool(same)}))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
