"""Inference harness: the counterpart of experiments/infer.py (`Tester`, :19-110) + experiments/eval.py's
registration report, on the native engine.

    python -m rdmnet_amd.infer --infer-root /path/to/assets/pc --out out/           # the two bundled pairs
    python -m rdmnet_amd.infer --dataset-root /data/kitti --subset test --out out/ --weights rdmnet.pth.tar
    python -m rdmnet_amd.infer --synthetic 512 --no-npz                              # throughput on synthetic KITTI-shaped pairs
    python -m rdmnet_amd.infer --dataset-root /data/kitti --gt-nodes --out out/      # test.py's evaluation run (eval.py reads out/)
    python -m rdmnet_amd.infer --infer-root /path/to/assets/pc --out out/ --feature-match mutual   # + descriptor correspondences
    python -m rdmnet_amd.infer --infer-root /path/to/assets/pc --out out/ --quality                # + fitness, inlier RMSE, chamfer
    python -m rdmnet_amd.infer --infer-root /path/to/assets/pc --out out/ --information            # + the 6 x 6 pose information matrix
    python -m rdmnet_amd.infer --infer-root /path/to/assets/pc --out out/ --robust                 # + the maximum-clique / GNC-TLS pose
    python -m rdmnet_amd.infer --dataset-root /data/kitti --pair-lists loops --information --out out/   # the loop pairs of `prepare loops`
    python -m torch.distributed.run --nproc-per-node 8 -m rdmnet_amd.infer ...       # pairs sharded over ranks

Per pair it writes what the reference writes: one line in `<seq>_pose` and one `<seq>_<src>_<ref>.npz`
(evaluation.save_pair_npz).  With ground truth in the loader it also prints eval.py's report lines.
Multi-GPU: rank r takes pairs r, r+W, ... (sharding.pairs_for_rank); the only collective is the final
gather of the per-pair records.  `--dataset mulran` switches the vote layer off as infer.py:119-120 does.
`--gt-nodes` turns the run into test.py's (eval.sh -> experiments/test.py, the model of experiments/model.py): for every pair
with a ground-truth `transform` the ground-truth superpoint correspondences (model.py:283-297) are computed on the GPU from
the engine's resident tensors, the Coarse Matching meters become real, and the .npz holds exactly test.py:80-90's keys.
`--feature-match MODE` adds the classical descriptor protocol (extract_correspondences_from_feats,
geotransformer/utils/registration.py:258-277, on the fine level: Engine.feature_correspondences) to every pair file --
evaluation.FEATURE_MATCH_KEYS, what `python -m rdmnet_amd.eval --method ransac_featurematch` reads -- and, with ground truth, the
descriptor inlier ratio to the pair's log line.
`--quality` judges every pair's pose without ground truth (Engine.alignment_quality on the resident input clouds, radius
cfg.fine_matching.acceptance_radius): fitness and inlier RMSE of both sides and the chamfer distance go to the pair's log line and,
as quality_* keys (ops.QUALITY_KEYS), into its .npz; every other key stays as it is.
`--information` says how well every pair's pose is constrained, for a pose graph: Open3D's 6 x 6 information matrix of the pair
(Engine.information_matrix on the resident input clouds, src moved by the pair's own pose against ref, radius
cfg.fine_matching.acceptance_radius) goes into the .npz as `information` (float64 [6, 6]) with `information_corr` (int64, the
correspondences behind it), and `info_corr: N` to the pair's log line; every other key stays as it is.
`--robust` adds an outlier-robust pose of every pair from its fine correspondences (ops.robust_registration: maximum clique of
the compatibility graph, GNC-TLS rotation, truncated-least-squares translation; --noise-bound, default 0.01, eval.py:200; the
16384 best-scored rows when there are more) to the .npz as `estimated_transform_robust` (float64 [4, 4]), and `robust_K` (rows it
was estimated from), `robust_exact` and, with ground truth, the pose's RRE / RTE to the pair's log line; every other key stays.
`--pair-lists NAME [--sequences ...]` takes the pairs from the lists R/NAME/%02d (the format of icp10: `src ref` + the pose) instead
of icp10 and --subset: with `loops`, the loop closures `python -m rdmnet_amd.prepare loops` detected, whose pair files
`python -m rdmnet_amd.trajectory --optimize` takes as loop edges.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from . import _lib, config, dataset as ds_mod, evaluation, ops, sharding, weights
from .pipeline import DEFAULT_PAIRS_IN_FLIGHT, PairPipeline, pin_rank


def load_state(path, cfg, seed=0):
    """`state['model']` of a reference checkpoint (base_tester.py:97-107), or synthetic weights."""
    if path:
        state = torch.load(path, map_location='cpu')
        return state['model'] if 'model' in state else state
    return weights.synthetic_state_dict(cfg, seed=seed)


class Tester:
    """`run(stager)` processes this rank's pairs with `pairs_in_flight` of them on the GPU at a time
    (rdmnet_amd.pipeline.PairPipeline: what replaces the one-pair-at-a-time loop of engine/single_tester.py:86-134);
    records, pose lines and the report come out in dataset order whatever the completion order."""

    def __init__(self, cfg, state, output_dir=None, save_npz=True, ransac=True, write_poses=True,
                 pairs_in_flight=DEFAULT_PAIRS_IN_FLIGHT, wait_us=None, lockstep=None, gt_nodes=False, feature_match=None,
                 quality=False, information=False, robust=False, noise_bound=0.01):
        self.cfg, self.output_dir, self.save_npz, self.ransac = cfg, output_dir, save_npz, ransac
        self.write_poses = write_poses  # False under several ranks: rank 0 writes all poses, in pair order, at the end
        # gt_nodes: test.py's run -- ground-truth superpoint correspondences per pair with a transform (model.py:283-297, radius
        # cfg.model.ground_truth_matching_radius, 0.6 when absent), the coarse meters, test.py:80-90's .npz
        self.gt_nodes = bool(gt_nodes)
        # feature_match: 'nearest' | 'mutual' | 'bilateral' -- the descriptor correspondences of the fine level per pair
        if feature_match is not None and feature_match not in ops.FEATURE_MATCH_MODES:
            raise ValueError(f'feature_match {feature_match!r}, expected one of {sorted(ops.FEATURE_MATCH_MODES)}')
        self.feature_match = feature_match
        self.quality = bool(quality)  # Engine.alignment_quality of every pair's own pose, on the input clouds
        self.information = bool(information)  # Engine.information_matrix of every pair's own pose, on the input clouds
        self.robust, self.noise_bound = bool(robust), float(noise_bound)  # ops.robust_registration on the fine correspondences
        ev = dict(cfg.get('eval', {})) if hasattr(cfg, 'get') else {}
        self.fm_radius = float(ev.get('acceptance_radius', 0.6))
        radius = getattr(getattr(cfg, 'model', None), 'ground_truth_matching_radius', None)
        self.gt_radius = 0.6 if radius is None else float(radius)
        self.pipeline = PairPipeline(cfg, state, pairs_in_flight=pairs_in_flight, wait_us=wait_us,
                                     keep_taps=bool(save_npz and output_dir) or self.gt_nodes, lockstep=lockstep)
        self.engine = self.pipeline.engines[0]  # (the serial entry point `step` runs on this one)
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        self.summary = evaluation.Summary()
        self.records = []

    @staticmethod
    def output_dict(e, n_ref):
        """The tensors infer.py:84-101 stores, from engine e's taps of its last run."""
        r = e.result
        lv0, lv1 = e.tensor('points0'), e.tensor('points1')
        nodes, feats = e.tensor('nodes'), e.tensor('feats_c')
        m_r, n_ref_f = int(r.n_ref_nodes), int(r.level_ref_sizes[1])
        rc, sc, cs = e.corr()
        out = {'ref_points': lv0[:n_ref], 'src_points': lv0[n_ref:],
               'ref_points_f': lv1[:n_ref_f], 'src_points_f': lv1[n_ref_f:],
               'ref_points_c': nodes[:m_r], 'src_points_c': nodes[m_r:],
               'ref_feats_c': feats[:m_r], 'src_feats_c': feats[m_r:],
               'ref_node_corr_indices': e.tensor('ref_node_corr_indices')[:, 0],
               'src_node_corr_indices': e.tensor('src_node_corr_indices')[:, 0],
               'ref_corr_points': rc, 'src_corr_points': sc, 'corr_scores': cs,
               'estimated_transform': torch.from_numpy(e.transform())}
        return out

    def _work(self, eng, job):
        """One pair on a worker thread / stream of the pipeline: run it and take everything the harness needs out of the
        engine (the next pair reuses its arena).  The .npz of a pair is an independent file: written here."""
        item, ref_dev, src_dev = job
        t0 = time.perf_counter()
        res = eng.run(ref_dev.contiguous(), src_dev.contiguous())  # returns with pose AND correspondences on the host
        ms = (time.perf_counter() - t0) * 1e3
        T = eng.transform()
        rec = {'seq_id': item['seq_id'], 'ref_frame': item['ref_frame'], 'src_frame': item['src_frame'],
               'n_corr': int(res.n_correspondences), 'ms': ms, 'transform': T}
        if 'transform' in item:  # what the pair's registration / correspondence numbers need (the engine's buffers are reused)
            rec['_measure'] = (np.asarray(item['transform'], np.float64), T) + eng.host_corr()  # (numpy copies)
        extra = None
        if self.feature_match:  # the descriptor protocol on the engine's resident fine points and features, this stream
            extra = evaluation.feature_match_arrays(eng.feature_correspondences('fine', self.feature_match))
            rec['n_feat_corr'] = int(extra['feat_corr_dists'].shape[0])
            if 'transform' in item and rec['n_feat_corr'] > 0:  # evaluate_correspondences on those points (registration.py:361-375)
                rec['feat_IR'] = float(evaluation.evaluate_correspondences(
                    extra['feat_ref_corr_points'], extra['feat_src_corr_points'], np.asarray(item['transform'], np.float64),
                    positive_radius=self.fm_radius)['inlier_ratio'])
        if self.quality:  # fitness / inlier RMSE / chamfer of the pair's own pose on the engine's resident input clouds, this stream
            rec['quality'] = eng.alignment_quality()
            extra = dict(extra or {})
            extra.update({f'quality_{k}': np.float64(rec['quality'][k]) for k in ops.QUALITY_KEYS})
        if self.information:  # the pose information matrix of the pair on the engine's resident input clouds, this stream
            info = eng.information_matrix()
            rec['info_corr'] = int(eng.information_corr)
            extra = dict(extra or {})
            extra.update(information=info.numpy(), information_corr=np.int64(rec['info_corr']))
        if self.robust:  # the outlier-robust pose from the pair's fine correspondences, this stream
            rc, sc, cs = eng.corr()
            if rc.shape[0] > _lib.ROBUST_MAX_CORR:  # the graph's capacity: the best-scored rows, as eval.py --num_corr selects
                from .eval import select_rows
                rows = torch.from_numpy(select_rows(cs.cpu().numpy(), _lib.ROBUST_MAX_CORR)).to(rc.device)
                rc, sc = rc[rows], sc[rows]
            rb = ops.robust_registration(sc.contiguous(), rc.contiguous(), noise_bound=self.noise_bound)
            rec['robust_K'], rec['robust_exact'] = rb.num_selected, rb.exact
            if 'transform' in item:
                rec['robust_RRE'], rec['robust_RTE'] = (float(v) for v in evaluation.compute_registration_error(
                    np.asarray(item['transform'], np.float64), rb.transformation)[:2])
            extra = dict(extra or {})
            extra.update(estimated_transform_robust=rb.transformation)
        if self.gt_nodes and 'transform' in item:  # test.py: model.py:283-297 on the engine's resident tensors, this stream
            gt_idx, gt_ovl, _ = eng.gt_node_correspondences(np.asarray(item['transform'], np.float32), self.gt_radius)
            m_r = int(res.n_ref_nodes)
            t = eng.tensors(['nodes', 'ref_node_corr_indices', 'src_node_corr_indices'])  # (one batched copy)
            nodes, r_sel, s_sel = (t[k].cpu().numpy() for k in ('nodes', 'ref_node_corr_indices', 'src_node_corr_indices'))
            rec['_nodes'] = (nodes[:m_r], nodes[m_r:], r_sel[:, 0], s_sel[:, 0], gt_idx.cpu().numpy())
            if self.output_dir and self.save_npz:
                od = self.output_dict(eng, item['ref_points'].shape[0])
                od.update(gt_node_corr_indices=gt_idx, gt_node_corr_overlaps=gt_ovl)
                evaluation.save_pair_test_npz(self.output_dir, item, od, extra=extra)
            return rec
        if self.output_dir and self.save_npz:
            od = self.output_dict(eng, item['ref_points'].shape[0])
            T_ransac = None
            if self.ransac:  # infer.py:75-82: distance 0.3, ransac_n 4, 50 000 iterations, on the GPU
                T_ransac = ops.ransac_correspondences(od['src_corr_points'].contiguous(), od['ref_corr_points'].contiguous(),
                                                      0.3, 4, 50000)[0].cpu().numpy().astype(np.float64)
            evaluation.save_pair_npz(self.output_dir, item, od, estimated_transform_ransac=T_ransac, extra=extra)
        return rec

    def _commit(self, rec):
        """In dataset order, on the calling thread: pose line, registration meters, record list."""
        if self.output_dir and self.write_poses:
            evaluation.append_pose(self.output_dir, rec, rec['transform'])
        args = rec.pop('_measure', None)
        nodes = rec.pop('_nodes', None)
        if args is not None:  # 0.3 ms of host work per pair: here it does not keep a worker's stream idle
            rec.update(self.summary.commit((rec['seq_id'], rec['src_frame'], rec['ref_frame']),
                                           self.summary.measure(*args, nodes=nodes)))
        self.records.append(rec)
        return rec

    def step(self, item, ref_dev, src_dev):
        """One pair, serially, on the calling thread's current stream."""
        return self._commit(self._work(self.engine, (item, ref_dev, src_dev)))

    def run(self, stager, log=None):
        """Every pair of the stager, `pairs_in_flight` at a time, committed in dataset order.  If a pair fails, the pairs before
        it are still committed (pose lines, records) before the error is raised; .npz files of later pairs that had already
        finished on other workers may exist without a pose line."""
        # (tensors_of: the pipeline's workers collate several staged pairs with one sequence of launches, pipeline.PairPipeline.imap)
        for i, rec in enumerate(self.pipeline.imap(stager, self._work, tensors_of=lambda job: (job[1].contiguous(), job[2].contiguous()))):
            # a pair's time: from the moment its worker drew it to its result (in a lock-step group the pairs finish together, and
            # `engine.run` in _work only picks the result up)
            rec['ms'] = self.pipeline.last_stats['latency_ms'].get(i, rec['ms'])
            self._commit(rec)
            if log:
                line = 'seq_id: {}, id0: {}, id1: {}, nCorr: {}'.format(rec['seq_id'], rec['ref_frame'], rec['src_frame'],
                                                                        rec['n_corr'])
                if 'n_feat_corr' in rec:  # (--feature-match)
                    line += ', nFeatCorr: {}'.format(rec['n_feat_corr'])
                    if 'feat_IR' in rec:
                        line += ', feat_IR: {:.3f}'.format(rec['feat_IR'])
                if 'quality' in rec:  # (--quality)
                    line += ''.join(', {}: {:.4f}'.format(k, rec['quality'][k]) for k in ops.QUALITY_KEYS)
                if 'info_corr' in rec:  # (--information)
                    line += ', info_corr: {}'.format(rec['info_corr'])
                if 'robust_K' in rec:  # (--robust)
                    line += ', robust_K: {}, robust_exact: {}'.format(rec['robust_K'], rec['robust_exact'])
                    if 'robust_RRE' in rec:
                        line += ', robust_RRE: {:.3f}, robust_RTE: {:.3f}'.format(rec['robust_RRE'], rec['robust_RTE'])
                log(line)
        return self.records


def pair_list_metadata(dataset_root, name, sequences=None):
    """The dataset metadata of the pair lists R/NAME/%02d (dataset.load_kitti_gt_txt: `src ref` + 12 pose values per line, e.g.
    what `prepare loops` writes under R/loops) -> (metadata, sequences).  sequences None: every list under R/NAME."""
    import glob
    folder = os.path.join(dataset_root, name)
    if sequences is None:
        sequences = sorted(int(os.path.basename(f)) for f in glob.glob(os.path.join(folder, '[0-9][0-9]')))
        if not sequences:
            raise FileNotFoundError(f'no pair lists under {folder}')
    metadata = []
    for seq in sequences:
        metadata += ds_mod.load_kitti_gt_txt(folder, int(seq))
    return metadata, [int(s) for s in sequences]


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--infer-root', default=None, help="directory with %%06d.npy scans of the 'infer' subset (assets/pc)")
    ap.add_argument('--dataset-root', default=None, help='KITTI-style root (icp10/<seq> lists + downsampled_xyzi/)')
    ap.add_argument('--subset', default='test')
    ap.add_argument('--dataset', default='kitti', help="'mulran' disables the vote layer (infer.py:119-120)")
    ap.add_argument('--weights', default=None, help='reference checkpoint (.pth.tar); default: synthetic seed-0 weights')
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-npz', action='store_true')
    ap.add_argument('--neighbor-limits', type=int, nargs=5, default=None, help='skip the calibration')
    ap.add_argument('--bf16-attention', action='store_true')
    ap.add_argument('--synthetic', type=int, default=0, metavar='N',
                    help='no dataset: N pairs cycling through the bench workload\'s seeded synthetic KITTI-shaped pairs '
                         '(rdmnet_amd.synthetic; --synthetic-distinct of them, cached under --synthetic-cache)')
    ap.add_argument('--synthetic-distinct', type=int, default=8)
    ap.add_argument('--synthetic-cache', default=os.path.join('gpurun_out', 'bench_pairs'))
    ap.add_argument('--pairs-in-flight', type=int, default=DEFAULT_PAIRS_IN_FLIGHT,
                    help='pairs on the GPU at a time (engines / host threads / HIP streams; rdmnet_amd.pipeline)')
    ap.add_argument('--lockstep', type=int, default=None,
                    help='pairs a stream runs as one lock-step group (identical kernels of the group as one grouped launch; default: '
                         'rdmnet_amd.pipeline.DEFAULT_LOCKSTEP with two or more pairs in flight and no .npz outputs; 1 = one pair per engine call)')
    ap.add_argument('--no-ransac', action='store_true', help='skip the RANSAC estimate stored beside the LGR pose in the .npz')
    ap.add_argument('--quiet', action='store_true', help='no per-pair log line (the reference prints one per iteration, infer.py:62-66)')
    ap.add_argument('--gt-nodes', action='store_true',
                    help="test.py's evaluation run: ground-truth superpoint correspondences on the GPU for every pair with a transform "
                         "(experiments/model.py:283-297), real Coarse Matching meters, .npz files with test.py's keys (eval.py reads them)")
    ap.add_argument('--feature-match', choices=sorted(ops.FEATURE_MATCH_MODES), default=None,
                    help='also match the fine-level descriptors by nearest neighbour in feature space (registration.py:222-277) and add '
                         'feat_ref/src_corr_indices, feat_ref/src_corr_points and feat_corr_dists to every pair file')
    ap.add_argument('--quality', action='store_true',
                    help="judge every pair's pose without ground truth: fitness and inlier RMSE of both clouds and the chamfer distance "
                         'at cfg.fine_matching.acceptance_radius, in the log line and as quality_* keys of the pair file')
    ap.add_argument('--information', action='store_true',
                    help="add every pair's 6 x 6 pose information matrix (Open3D's get_information_matrix_from_point_clouds at "
                         'cfg.fine_matching.acceptance_radius, for a pose graph) to the pair file as information / information_corr')
    ap.add_argument('--robust', action='store_true',
                    help="add every pair's outlier-robust pose from its fine correspondences (maximum clique, GNC-TLS rotation, "
                         'truncated-least-squares translation) to the pair file as estimated_transform_robust')
    ap.add_argument('--noise-bound', '--noise_bound', type=float, default=0.01, help='noise bound of --robust (eval.py:200)')
    ap.add_argument('--pair-lists', default=None, metavar='NAME',
                    help='with --dataset-root: the pairs of the lists R/NAME/%%02d instead of icp10 and --subset, e.g. `loops` (what '
                         '`python -m rdmnet_amd.prepare loops` writes); the pair files are the loop edges trajectory --optimize takes')
    ap.add_argument('--sequences', type=int, nargs='+', default=None, help='the sequences of --pair-lists (default: every list there)')
    return ap


def main(argv=None):
    ap = make_parser()
    args = ap.parse_args(argv)
    if (args.pair_lists or args.sequences) and not (args.pair_lists and args.dataset_root):
        ap.error('--pair-lists needs --dataset-root, --sequences needs --pair-lists')
    if args.pair_lists and (args.infer_root or args.synthetic > 0):
        ap.error('--pair-lists cannot be combined with --infer-root or --synthetic (they would take the pairs from elsewhere)')

    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    local_rank, local_world = int(os.environ.get('LOCAL_RANK', 0)), int(os.environ.get('LOCAL_WORLD_SIZE', world))
    pin_rank(local_rank, local_world)  # the CPUs of this rank's GPU's NUMA node (before the first HIP call)
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group('nccl')
    cfg = config.make_cfg()
    if args.dataset == 'mulran':
        cfg.Vote.inference_use_vote = False
    cfg.thdroformer.attention_bf16 = bool(args.bf16_attention)
    b = cfg.backbone
    if args.synthetic > 0:
        from . import synthetic
        fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'synthetic_pairs.npz')
        base = ds_mod.ArrayPairDataset(synthetic.cached_pairs(args.synthetic_distinct, args.synthetic_cache, fixture))
        data = ds_mod.CyclingPairDataset(base, args.synthetic)
        calib = base
    elif args.infer_root:
        data = ds_mod.OdometryKittiPairDataset('.', 'infer', infer_root=args.infer_root)
        calib = data
    elif args.dataset_root and args.pair_lists:
        metadata, _ = pair_list_metadata(args.dataset_root, args.pair_lists, args.sequences)
        data = ds_mod.OdometryKittiPairDataset(args.dataset_root, 'test', metadata=metadata)  # (any subset but 'infer': the lists' poses are used)
        calib = data
    elif args.dataset_root:
        data = ds_mod.OdometryKittiPairDataset(args.dataset_root, args.subset)
        calib = data
    else:
        ap.error('give --infer-root, --dataset-root or --synthetic N')
    t0 = time.time()
    if args.neighbor_limits:
        cfg.neighbor_limits = list(args.neighbor_limits)
    else:
        cfg.neighbor_limits = [int(x) for x in ds_mod.calibrate_neighbors_stack_mode(
            calib, None, b.num_stages, b.init_voxel_size, b.init_radius)]
    if rank == 0:
        print(f'Data loader created: {time.time() - t0:.3f}s collapsed.')
        print(f'Calibrate neighbors: {cfg.neighbor_limits}.')
    tester = Tester(cfg, load_state(args.weights, cfg), args.out, save_npz=not args.no_npz, ransac=not args.no_ransac,
                    write_poses=world == 1, pairs_in_flight=args.pairs_in_flight, lockstep=args.lockstep, gt_nodes=args.gt_nodes,
                    feature_match=args.feature_match, quality=args.quality,
                    information=args.information, robust=args.robust, noise_bound=args.noise_bound)
    mine = sharding.pairs_for_rank(len(data), rank, world)
    # scans are read and staged (pinned host -> HBM on a side stream) two pairs ahead of every in-flight pair
    stager = ds_mod.PairStager(data, mine, depth=2 * args.pairs_in_flight, workers=max(2, args.pairs_in_flight))
    t_run = time.perf_counter()
    records = tester.run(stager, log=print if rank == 0 and not args.quiet else None)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t_run
    # one gather of fixed-size records: ids, counts, time, errors, the pose (12 floats) and the pair's dataset index
    rec = torch.tensor([[r['seq_id'], r['ref_frame'], r['src_frame'], r['n_corr'], r['ms'], r.get('r_RRE', float('nan')),
                         r.get('r_RTE', float('nan')), *np.asarray(r['transform'], np.float64).reshape(-1)[:12], idx]
                        for r, idx in zip(records, mine)], dtype=torch.float64, device='cuda').reshape(-1, 20)
    allrec = torch.cat(sharding.gather_records(rec, world, dist)).cpu().numpy()
    if rank == 0:
        allrec = allrec[np.argsort(allrec[:, 19], kind='stable')]  # dataset order, whatever the rank count
        if world > 1 and args.out:  # the single-rank file, not a rank-interleaved one (evaluation.pose_line format)
            for row in allrec:
                evaluation.append_pose(args.out, {'seq_id': int(row[0]), 'ref_frame': int(row[1]), 'src_frame': int(row[2])},
                                       row[7:19].astype(np.float32))
        print(f'pairs: {allrec.shape[0]}, mean ms/pair: {allrec[:, 4].mean() if len(allrec) else 0:.2f}, '
              f'{allrec.shape[0] / max(t_run, 1e-9):.1f} pairs/s (rank 0 wall time {t_run:.2f} s: host scans -> staging -> '
              f'{tester.pipeline.n} streams x {tester.pipeline.lockstep} pair(s) per lock-step group in flight -> poses and correspondences on the host)')
        st = tester.pipeline.last_stats
        if st and st['jobs']:
            print('  worker time per pair (ms): drawing + staging the next pair {:.2f}, engine + outputs {:.2f}, waiting for the '
                  'in-order consumer {:.2f}'.format(*(1e3 * st[k] / st['jobs'] for k in ('draw_s', 'work_s', 'window_s'))))
        if len(allrec) and np.isfinite(allrec[:, 5]).any():
            ok = (allrec[:, 5] < tester.summary.rre_threshold) & (allrec[:, 6] < tester.summary.rte_threshold)
            print('  Registration (all ranks), RR: {:.4f}, RRE: {:.3f}, RTE: {:.3f}'.format(
                ok.mean(), allrec[ok, 5].mean() if ok.any() else 0.0, allrec[ok, 6].mean() if ok.any() else 0.0))
            if world == 1:  # correspondence-level meters (PIR / IR / FMR) are accumulated per rank only
                for line in tester.summary.lines()[0 if args.gt_nodes else 1:]:  # (the coarse meters exist with --gt-nodes)
                    print(line)
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
