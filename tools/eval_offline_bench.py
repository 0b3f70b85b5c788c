"""Wall time of the offline evaluation over one directory of pair files: the host path (evaluation.Summary.measure / commit per
file, a pool of 16 threads as the inference harness runs it, and a plain loop) against `python -m rdmnet_amd.eval --method lgr`
(rdm_eval_pairs).  The directory is the fixture pairs of tests/golden/eval_pairs.npz written --copies times.

    python tools/eval_offline_bench.py [--copies 72] [--batch 64] [--repeats 3]

Prints one JSON line: seconds including file loading, and the evaluation alone (host: measure + commit on loaded arrays; GPU:
the time inside ops.evaluate_pairs, copies included)."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rdmnet_amd import eval as cli, evaluation  # noqa: E402

KEYS = ('ref_points_c', 'src_points_c', 'ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points', 'src_corr_points',
        'corr_scores', 'gt_node_corr_indices', 'gt_node_corr_overlaps', 'transform', 'estimated_transform')


def write_pairs(root, copies):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'eval_pairs.npz'))
    n = 0
    for c in range(copies):
        for k, name in enumerate(z['names']):
            np.savez_compressed(os.path.join(root, f'{c}_{k}_{k + 1}.npz'), **{key: z[f'{name}/{key}'] for key in KEYS})
            n += 1
    return n


def load(name):
    with np.load(name) as z:
        return {k: z[k] for k in KEYS}


def measure(summary, d):
    nodes = (d['ref_points_c'], d['src_points_c'], d['ref_node_corr_indices'], d['src_node_corr_indices'], d['gt_node_corr_indices'])
    return summary.measure(d['transform'], d['estimated_transform'], d['ref_corr_points'], d['src_corr_points'], d['corr_scores'], nodes)


def host_path(root, threads):
    _, todo = cli.list_pairs(root)
    summary = evaluation.Summary()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for (_, _, ids), m in zip(todo, pool.map(lambda item: measure(summary, load(item[1])), todo)):
            summary.commit(ids, m)
    total = time.perf_counter() - t0
    data = [load(name) for _, name, _ in todo]
    summary = evaluation.Summary()
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for (_, _, ids), m in zip(todo, pool.map(lambda d: measure(summary, d), data)):
            summary.commit(ids, m)
    return total, time.perf_counter() - t0, summary.lines()


def gpu_path(root, batch):
    args = cli.make_parser().parse_args(['--features-root', root, '--batch', str(batch)])
    timings, lines = {}, []
    t0 = time.perf_counter()
    cli.evaluate(args, emit=lines.append, timings=timings)
    return time.perf_counter() - t0, timings, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--copies', type=int, default=72)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        n = write_pairs(root, a.copies)
        gpu_path(root, a.batch)  # warm-up: library load, allocator, page cache
        out = {'pairs': n, 'batch': a.batch, 'host_16_threads': [], 'host_1_thread': [], 'gpu': []}
        for _ in range(a.repeats):
            for key, threads in (('host_16_threads', 16), ('host_1_thread', 1)):
                total, only, host_lines = host_path(root, threads)
                out[key].append({'wall_s': round(total, 4), 'evaluation_only_s': round(only, 4)})
            total, t, gpu_lines = gpu_path(root, a.batch)
            out['gpu'].append({'wall_s': round(total, 4), 'evaluation_only_s': round(t['evaluate'], 4),
                               'waiting_for_files_s': round(t['load_wait'], 4)})
        out['report_equal'] = gpu_lines[1:] == host_lines
        print(json.dumps(out))


if __name__ == '__main__':
    main()
