"""Offline evaluator: experiments/eval.py on the GPU.

    python -m rdmnet_amd.eval --features-root DIR [--method lgr|ransac|svd|ransac_featurematch|robust] [--num_corr N] [--verbose]
                              [--batch B] [--noise-bound B] [--inlier-selection clique|kcore|none]

reads the pair files `python -m rdmnet_amd.infer --gt-nodes` (or the reference's test.py) wrote into DIR and prints the
report of eval.py:248-286.  Files are ordered as eval.py:78-81 orders them, pair (seq 8, src frame 15) is skipped as in
:94-95.  Reader threads load, decompress and pack the next batches while the current one is evaluated by
`ops.evaluate_pairs` (one host-to-device copy, a fixed number of kernel launches and one device-to-host copy per batch).
The `Node Detection` line prints zeros: the reference registers its meters and never updates them.

`--method ransac_featurematch` is THIS project's definition: the reference's parser accepts the name (eval.py:30) and its loop has
no branch for it (eval.py:177-219).  The pair is evaluated on the descriptor correspondences `infer --feature-match` stored
(feat_ref/src_corr_points) in place of ref/src_corr_points, with score -feat_corr_dists -- so --num_corr N keeps the N smallest
feature distances, lowest rows among equals --, the fine meters are the descriptor IR / FMR, and the pose is
rdm_ransac_correspondences with the cfg.ransac values, as --method ransac.  Open3D's own
registration_ransac_based_on_feature_matching (its internal KNN and checkers) is not restated.

`--method robust` is THIS project's definition of the estimator eval.py:198-219 calls `teaser` (maximum clique
of the compatibility graph, GNC-TLS rotation, truncated-least-squares translation; the library eval.py imports is not part of
the reference tree, and the name `teaser` stays rejected).  The host selects the --num_corr rows by rdm_eval_pairs' own rule
(score descending, row ascending, the first N, kept in row order), `ops.robust_registration` runs once per pair with
--noise-bound (default 0.01, eval.py:200) and --inlier-selection, and the pairs are then evaluated as --method lgr with the
computed transforms in place of the stored ones.
"""
import argparse
import glob
import os.path as osp
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import config, evaluation

METHODS = ('lgr', 'ransac', 'svd')                # what the reference's evaluation loop implements (eval.py:177-219)
OWN_METHODS = ('ransac_featurematch',)            # defined by this project; the command line takes them (main)
ROBUST_METHODS = ('robust',)                      # this project's maximum-clique / GNC-TLS estimator (ops.robust_registration)
NOT_BUILT = {'teaser': "TEASER++ is not part of this project; its algorithm, as this project defines it, is --method robust",
             'robust': 'this project\'s own estimator is enabled by make_parser(own_methods=True), as the command line does',
             'ransac_featurematch': "the reference's evaluation loop has no branch for it (eval.py:177-219); this project's "
                                    "definition is enabled by make_parser(own_methods=True), as the command line does"}
FEATURE_KEYS = ('feat_ref_corr_points', 'feat_src_corr_points', 'feat_corr_dists')  # read by --method ransac_featurematch
PAIR_KEYS = ('ref_corr_points', 'src_corr_points', 'corr_scores', 'transform', 'estimated_transform', 'ref_node_corr_indices',
             'src_node_corr_indices', 'gt_node_corr_indices')
KERNEL_METHOD = {'ransac_featurematch': 'ransac', 'robust': 'lgr'}  # (rdm_eval_pairs is unchanged: only the packed rows differ)
MAX_THREADS = 16
# experiments/config.py: cfg.eval and cfg.ransac (a cfg that carries these sections overrides them)
EVAL_DEFAULTS = dict(acceptance_radius=0.6, inlier_ratio_threshold=0.05, rre_threshold=5.0, rte_threshold=2.0)
RANSAC_DEFAULTS = dict(distance_threshold=0.3, num_points=4, num_iterations=50000)


def method_arg(value, methods=METHODS):
    if value in methods:
        return value
    if value in NOT_BUILT:
        raise argparse.ArgumentTypeError(f"method '{value}' is not supported: {NOT_BUILT[value]}")
    raise argparse.ArgumentTypeError(f"invalid choice: '{value}' (choose from {', '.join(methods)})")


def make_parser(own_methods=False):
    """The reference's eval.py arguments.  own_methods: --method also takes OWN_METHODS (this project's definitions of names the
    reference advertises without implementing them); `python -m rdmnet_amd.eval` sets it."""
    methods = METHODS + OWN_METHODS + ROBUST_METHODS if own_methods else METHODS
    parser = argparse.ArgumentParser(prog='python -m rdmnet_amd.eval', description=__doc__.split('\n\n')[0])
    parser.add_argument('--features-root', '--features_root', required=True, help='directory of the {seq}_{src}_{ref}.npz pair files')
    parser.add_argument('--test_epoch', default=None, type=int, help='test epoch')
    parser.add_argument('--method', type=lambda v: method_arg(v, methods), default='lgr',
                        help='registration method: ' + ', '.join(methods))
    parser.add_argument('--num_corr', type=int, default=None, help='number of correspondences for registration')
    parser.add_argument('--verbose', action='store_true', help='verbose mode')
    parser.add_argument('--batch', type=int, default=64, help='pairs per GPU call')
    parser.add_argument('--workers', type=int, default=8, help=f'reader threads (at most {MAX_THREADS})')
    parser.add_argument('--seed', type=int, default=0, help='seed of --method ransac')
    if own_methods:
        parser.add_argument('--noise-bound', '--noise_bound', type=float, default=0.01, help='noise bound of --method robust')
        parser.add_argument('--inlier-selection', '--inlier_selection', choices=('clique', 'kcore', 'none'), default='clique',
                            help='inlier selection of --method robust')
    return parser


def split_name(file_name):
    return osp.splitext(osp.basename(file_name))[0].split('_')


def sort_key(file_name):
    """eval.py:80: the integers of the file name.  Names whose sequence id is not an integer (:87-90 reads those too) come
    after the integer ones, by (sequence id, src frame, ref frame)."""
    parts = split_name(file_name)
    try:
        return (0, [int(i) for i in parts], '')
    except ValueError:
        return (1, [int(i) for i in parts[1:]], parts[0])


def pair_ids(file_name):
    """eval.py:85-90 -> (seq_id, src_frame, ref_frame)."""
    parts = split_name(file_name)
    try:
        seq_id, src_frame, ref_frame = [int(x) for x in parts]
    except ValueError:
        seq_id, src_frame, ref_frame = parts
        src_frame, ref_frame = int(src_frame), int(ref_frame)
    return seq_id, src_frame, ref_frame


def list_pairs(features_root):
    """-> (number of files, [(position from 1, file name, ids)] without the pair eval.py:94-95 drops)."""
    names = sorted(glob.glob(osp.join(features_root, '*.npz')), key=lambda n: (sort_key(n)[0], sort_key(n)[2], sort_key(n)[1]))
    out = []
    for i, name in enumerate(names):
        ids = pair_ids(name)
        if ids[0] == 8 and ids[1] == 15:  # "delete bad data"
            continue
        out.append((i + 1, name, ids))
    return len(names), out


def load_pair(file_name, method='lgr'):
    with np.load(file_name) as z:
        d = {k: z[k] for k in PAIR_KEYS}
        d['node_dims'] = (z['ref_points_c'].shape[0], z['src_points_c'].shape[0])
        if method == 'ransac_featurematch':  # the stored descriptor correspondences take the place of the fine matching's
            for k in FEATURE_KEYS:
                if k not in z.files:
                    raise KeyError(f"{file_name} has no '{k}': --method ransac_featurematch reads the descriptor correspondences "
                                   "that `python -m rdmnet_amd.infer --feature-match {nearest,mutual,bilateral}` writes")
            d['ref_corr_points'] = np.ascontiguousarray(z['feat_ref_corr_points'], np.float32)
            d['src_corr_points'] = np.ascontiguousarray(z['feat_src_corr_points'], np.float32)
            d['corr_scores'] = -np.ascontiguousarray(z['feat_corr_dists'], np.float32)
    return d


def select_rows(scores, num_corr):
    """rdm_eval_pairs' rule for --num_corr L on the host: the first L rows in the order (score descending, row ascending), kept
    in row order; every row for L None or C <= L."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    if num_corr is None or len(scores) <= num_corr:
        return np.arange(len(scores))
    order = np.lexsort((np.arange(len(scores)), -scores.astype(np.float64)))  # last key first: score, then row
    return np.sort(order[:num_corr])


def robust_transforms(pairs, num_corr=None, noise_bound=0.01, inlier_selection='clique', results=None):
    """One ops.robust_registration per pair dict (load_pair) on its --num_corr rows -> float32 [P, 4, 4].  results (list):
    receives the RobustResult of every pair."""
    import torch
    from . import ops
    out = np.zeros((len(pairs), 4, 4), np.float32)
    for p, d in enumerate(pairs):
        rows = select_rows(d['corr_scores'], num_corr)
        src = torch.from_numpy(np.ascontiguousarray(np.asarray(d['src_corr_points'], np.float32).reshape(-1, 3)[rows])).cuda()
        ref = torch.from_numpy(np.ascontiguousarray(np.asarray(d['ref_corr_points'], np.float32).reshape(-1, 3)[rows])).cuda()
        res = ops.robust_registration(src, ref, noise_bound=noise_bound, inlier_selection=inlier_selection)
        out[p] = res.transformation.astype(np.float32)
        if results is not None:
            results.append(res)
    return out


def pair_message(position, total, ids, out):
    """eval.py:127,170-174,238-239."""
    m = '{}/{}, seq_id: {}, id0: {}, id1: {}'.format(position, total, *ids)
    m += ', c_PIR: {:.3f}'.format(out['c_PIR'])
    if 'f_IR' in out:
        m += ', f_IR: {:.3f}, f_OV: {:.3f}, f_RS: {:.3f}, f_NU: {}'.format(out['f_IR'], out['f_OV'], out['f_RS'], out['f_NU'])
    return m + ', r_RRE: {:.3f}, r_RTE: {:.3f}'.format(out['r_RRE'], out['r_RTE'])


def evaluate(args, cfg=None, emit=print, timings=None, collect=None):
    """eval_one_epoch (eval.py:36-286).  Returns the Summary.  `timings` (dict) receives the seconds the main thread spent
    waiting for packed batches ('load_wait') and inside the GPU calls ('evaluate'); `collect` (list) receives per pair
    (ids, record, the transform the record was computed with)."""
    import time
    from . import ops
    cfg = cfg or config.make_cfg()
    ev = dict(EVAL_DEFAULTS, **cfg.get('eval', {}))
    rs = dict(RANSAC_DEFAULTS, **cfg.get('ransac', {}))
    summary = evaluation.Summary(ev['acceptance_radius'], ev['inlier_ratio_threshold'], ev['rre_threshold'], ev['rte_threshold'])
    total, todo = list_pairs(args.features_root)
    batch = max(1, int(args.batch))
    workers = max(1, min(MAX_THREADS, int(args.workers)))
    batches = [todo[i:i + batch] for i in range(0, len(todo), batch)]
    t_wait = t_eval = 0.0
    with ThreadPoolExecutor(max_workers=workers) as pool:
        def prepare(items):  # files in parallel, then one packed buffer
            pairs = list(pool.map(lambda name: load_pair(name, args.method), [name for _, name, _ in items]))
            return (pairs if args.method in ROBUST_METHODS else None), ops.pack_eval_pairs(pairs)

        with ThreadPoolExecutor(max_workers=1) as packer:
            ahead = 2
            pending = [packer.submit(prepare, b) for b in batches[:ahead]]
            for k, items in enumerate(batches):
                t0 = time.perf_counter()
                pairs, packed = pending.pop(0).result()
                if k + ahead < len(batches):
                    pending.append(packer.submit(prepare, batches[k + ahead]))
                t1 = time.perf_counter()
                if pairs is not None:  # --method robust: the computed transforms take the place of the stored ones
                    est = robust_transforms(pairs, args.num_corr, args.noise_bound, args.inlier_selection)
                    o, dtype, shape = packed.sections['est_transform']
                    packed.buf.numpy()[o:o + est.nbytes] = est.reshape(-1).view(np.uint8)
                records, used = ops.evaluate_pairs(packed, KERNEL_METHOD.get(args.method, args.method), args.num_corr, acceptance_radius=ev['acceptance_radius'],
                                                distance_threshold=rs['distance_threshold'], ransac_n=rs['num_points'],
                                                num_iterations=rs['num_iterations'], seed=args.seed)
                t2 = time.perf_counter()
                t_wait += t1 - t0
                t_eval += t2 - t1
                for k2, ((position, _, ids), rec) in enumerate(zip(items, records)):
                    out = summary.commit_record(ids, rec)
                    if collect is not None:
                        collect.append((ids, rec, used[k2]))
                    if args.verbose:
                        emit(pair_message(position, total, ids, out))
    if timings is not None:
        timings.update(load_wait=t_wait, evaluate=t_eval, pairs=len(todo))
    if args.test_epoch is not None:
        emit(f'Epoch {args.test_epoch}, method {args.method}')
    for line in summary.report_lines():
        emit(line)
    return summary


def main(argv=None):
    args = make_parser(own_methods=True).parse_args(argv)
    if not osp.isdir(args.features_root):
        sys.exit(f'{args.features_root}: not a directory')
    evaluate(args)


if __name__ == '__main__':
    main()
