"""GPU: ops.evaluate_pairs (rdm_eval_pairs) and `python -m rdmnet_amd.eval` against the reference's recorded results
(tests/golden/eval_pairs.npz) and, for constructed pairs, against the float64 restatement (tests/eval_restatement.py).

Bounds.  Counts (inliers at the three radii, overlapping rows): equal to the reference's on every decided row -- a row whose
float64 distance lies within 1e-5 relative of the radius may fall either way, and the generator asserted that those are at most
1 % of a pair's rows.  Residual mean: 1e-4 m (a k = 3 fp32 chain plus translation at <= 80 m is <= ~4 ulp = 3e-5 m per axis).
RRE / RTE: 1e-9 of the float64 formulas on the same fp32 matrices.  svd pose: 1e-3 degrees and 1e-4 m of the reference's fp32
Procrustes, 1e-5 m of the float64 one (DESIGN.md 7's LGR bounds, the angle measured as there: tie_aware.rre_rte)."""
import os

import numpy as np
import pytest

import eval_restatement as R
import tie_aware

pytestmark = pytest.mark.gpu

FILE_KEYS = ('ref_points_c', 'src_points_c', 'ref_node_corr_indices', 'src_node_corr_indices', 'ref_corr_points',
             'src_corr_points', 'corr_scores', 'gt_node_corr_indices', 'gt_node_corr_overlaps', 'transform', 'estimated_transform')
THRESHOLDS = ('inlier_ratio', 'inlier_ratio_0.3', 'inlier_ratio_0.1', 'overlap')
COUNTS = ('inliers', 'inliers_0.3', 'inliers_0.1', 'overlap_rows')


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, 'eval_pairs.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def ops():
    import torch
    assert torch.cuda.is_available()
    from rdmnet_amd import ops
    return ops


def pair_of(fx, name):
    return {k: fx[f'{name}/{k}'] for k in FILE_KEYS}


def named(record):
    from rdmnet_amd import _lib
    return dict(zip(_lib.EVAL_FIELDS, record))


def accepted(rre, rte):
    return bool(rre < 5.0 and rte < 2.0)


def check_against_restatement(rec, pair, num_corr, transform, radius=0.6, where=''):
    """Everything of one record but the choice of the transform, against the float64 restatement on the same rows."""
    r = named(rec)
    want = R.evaluate(pair, 'lgr', num_corr, radius, est_transform=transform)
    f = want['fine']
    n = f['num_corr']
    assert r['num_corr'] == n, where
    for key, cnt in zip(THRESHOLDS, COUNTS):
        print(where, key, 'count', r[cnt], 'decided', f[key]['lo'], 'undecided', f[key]['undecided'])
        assert f[key]['lo'] <= r[cnt] <= f[key]['lo'] + f[key]['undecided'], (where, key)
        if n:
            assert r[key] == r[cnt] / n
    if n:
        print(where, 'residual', r['residual'], f['residual'])
        assert abs(r['residual'] - f['residual']) < 1e-4, where
    else:
        assert all(np.isnan(r[k]) for k in ('residual',) + THRESHOLDS)
    hit, pred, gt, precision = want['coarse']
    assert (r['hit_cells'], r['pred_cells'], r['gt_cells']) == (hit, pred, gt), where
    assert abs(r['precision'] - precision) < 1e-12
    err = want['registration']
    print(where, 'rre/rte', r['rre'], r['rte'], err[:2])
    assert abs(r['rre'] - err[0]) < 1e-9 and abs(r['rte'] - err[1]) < 1e-9, where
    assert all(abs(r[k] - e) < 1e-9 for k, e in zip(('rx', 'ry', 'rz'), err[2:])), where


@pytest.mark.parametrize('nc', [0, 250, 1000])
def test_lgr_on_the_fixture(fx, ops, nc):
    names = [str(n) for n in fx['names']]
    pairs = [pair_of(fx, n) for n in names]
    records, transforms = ops.evaluate_pairs(pairs, 'lgr', nc or None)
    for name, pair, rec, T in zip(names, pairs, records, transforms):
        p = f'{name}/nc{nc}/'
        r = named(rec)
        ov, ir, ir3, ir1, res, n = fx[p + 'fine']
        assert r['num_corr'] == n == len(fx[p + 'sel'])
        for i, cnt in enumerate(COUNTS):
            lo, und = fx[p + 'lo'][i], fx[p + 'undecided'][i]
            print(name, nc, cnt, r[cnt], 'reference', round((ir, ir3, ir1, ov)[i] * n), 'decided', lo, 'undecided', und)
            assert lo <= r[cnt] <= lo + und and und <= 0.01 * n, (name, cnt)
            assert r[THRESHOLDS[i]] == r[cnt] / n
        print(name, nc, 'residual', r['residual'], res)
        assert abs(r['residual'] - res) < 1e-4
        assert abs(r['precision'] - fx[f'{name}/precision']) < 1e-12
        err = fx[p + 'err_lgr']
        print(name, nc, 'rre', r['rre'], err[0], 'rte', r['rte'], err[1])
        assert abs(r['rre'] - err[0]) < 1e-9 and abs(r['rte'] - err[1]) < 1e-9
        assert all(abs(r[k] - e) < 1e-9 for k, e in zip(('rx', 'ry', 'rz'), err[2:]))
        assert accepted(r['rre'], r['rte']) == bool(fx[p + 'accepted'][0])
        assert np.array_equal(T, pair['estimated_transform'])
        check_against_restatement(rec, pair, nc or None, T, where=f'{name} nc{nc}')


@pytest.mark.parametrize('nc', [0, 250, 1000])
def test_svd_on_the_fixture(fx, ops, nc):
    names = [str(n) for n in fx['names']]
    pairs = [pair_of(fx, n) for n in names]
    records, transforms = ops.evaluate_pairs(pairs, 'svd', nc or None)
    for name, pair, rec, T in zip(names, pairs, records, transforms):
        p = f'{name}/nc{nc}/'
        rows = R.select(pair['corr_scores'], nc or None)
        exact = R.weighted_procrustes(pair['src_corr_points'][rows], pair['ref_corr_points'][rows], pair['corr_scores'][rows])
        rre, rte = tie_aware.rre_rte(T, fx[p + 'svd_transform'])
        rre64, rte64 = tie_aware.rre_rte(T, exact)
        print(name, nc, 'vs reference', rre, rte, 'vs float64', rre64, rte64)
        assert rre < 1e-3 and rte < 1e-4
        assert rre64 < 1e-3 and rte64 < 1e-5
        assert np.array_equal(T[3], [0, 0, 0, 1])
        r = named(rec)
        assert accepted(r['rre'], r['rte']) == bool(fx[p + 'accepted'][1])
        check_against_restatement(rec, pair, nc or None, T, where=f'{name} svd nc{nc}')


@pytest.mark.parametrize('nc', [0, 250])
def test_ransac_uses_the_transform_of_ransac_correspondences(fx, ops, nc):
    import torch
    names = [str(n) for n in fx['names']]
    pairs = [pair_of(fx, n) for n in names]
    records, transforms = ops.evaluate_pairs(pairs, 'ransac', nc or None, seed=7)
    for name, pair, rec, T in zip(names, pairs, records, transforms):
        rows = R.select(pair['corr_scores'], nc or None)
        src = torch.from_numpy(np.ascontiguousarray(pair['src_corr_points'][rows])).cuda()
        ref = torch.from_numpy(np.ascontiguousarray(pair['ref_corr_points'][rows])).cuda()
        want = ops.ransac_correspondences(src, ref, 0.3, 4, 50000, seed=7)[0].cpu().numpy()
        assert np.array_equal(T, want), name
        check_against_restatement(rec, pair, nc or None, T, where=f'{name} ransac nc{nc}')


def constructed_pair(seed, c, noise=0.05, m=40, n=50):
    """A pair with a usable pose: src is ref moved back by the ground truth plus noise that grows along the rows."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = rot, rng.uniform(-5, 5, 3)
    ref = rng.uniform(-40, 40, (c, 3))
    spread = noise * (1 + 40 * np.arange(c)[:, None] / max(c, 1))
    src = (ref - gt[:3, 3]) @ rot + rng.normal(size=(c, 3)) * spread
    est = gt.copy()
    est[:3, 3] += [0.02, -0.01, 0.03]
    pred = np.stack([rng.integers(0, m, 256), rng.integers(0, n, 256)], 1)
    pred[200:] = pred[:56]  # repeated cells
    gt_idx = np.concatenate([pred[:90], pred[:30], np.stack([rng.integers(0, m, 200), rng.integers(0, n, 200)], 1)])
    return {'ref_corr_points': ref.astype(np.float32), 'src_corr_points': src.astype(np.float32),
            'corr_scores': rng.random(c).astype(np.float32), 'transform': gt.astype(np.float32),
            'estimated_transform': est.astype(np.float32), 'ref_node_corr_indices': pred[:, 0], 'src_node_corr_indices': pred[:, 1],
            'gt_node_corr_indices': gt_idx, 'node_dims': (m, n)}


@pytest.mark.parametrize('method', ['lgr', 'svd'])
def test_num_corr_boundary_inside_equal_scores_keeps_the_lowest_rows(ops, method):
    pair = constructed_pair(1, 1500)
    scores = pair['corr_scores']
    scores[100:1400:2] = np.float32(0.625)  # 650 equal scores; about 180 rows score higher
    above = int((scores > 0.625).sum())
    nc = above + 200
    rows = R.select(scores, nc)
    assert (scores[rows] == np.float32(0.625)).sum() == 200 and rows[scores[rows] == np.float32(0.625)].max() == 100 + 2 * 199
    records, transforms = ops.evaluate_pairs([pair], method, nc)
    check_against_restatement(records[0], pair, nc, transforms[0], where=f'tie {method}')
    if method == 'svd':  # the pose is that of exactly these rows (the noise grows along the rows: other rows, other pose)
        exact = R.weighted_procrustes(pair['src_corr_points'][rows], pair['ref_corr_points'][rows], scores[rows])
        rre, rte = tie_aware.rre_rte(transforms[0], exact)
        assert rre < 1e-3 and rte < 1e-5, (rre, rte)
        r = named(records[0])
        assert accepted(r['rre'], r['rte'])


@pytest.mark.parametrize('method', ['lgr', 'svd', 'ransac'])
def test_pairs_with_no_and_one_correspondence(ops, method):
    empty, single, full = constructed_pair(2, 0), constructed_pair(3, 1), constructed_pair(4, 300)
    records, transforms = ops.evaluate_pairs([empty, single, full], method, 100, seed=3)
    assert named(records[0])['num_corr'] == 0 and named(records[1])['num_corr'] == 1 and named(records[2])['num_corr'] == 100
    for k, pair in enumerate((empty, single, full)):
        check_against_restatement(records[k], pair, 100, transforms[k], where=f'C={len(pair["corr_scores"])} {method}')
    if method != 'lgr':
        assert np.array_equal(transforms[0], np.eye(4, dtype=np.float32))  # nothing to fit: identity
    if method == 'svd':
        # one row: the covariance has rank 1, which fixes the image of the row's direction and the translation, not the rotation
        exact = R.weighted_procrustes(single['src_corr_points'], single['ref_corr_points'], single['corr_scores'])
        T = transforms[1].astype(np.float64)
        assert np.abs(T[:3, 3] - exact[:3, 3]).max() < 1e-5
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-6 and np.linalg.det(T[:3, :3]) > 0.999
        a, b = single['src_corr_points'][0].astype(np.float64), single['ref_corr_points'][0].astype(np.float64)
        assert np.abs(T[:3, :3] @ (a / np.linalg.norm(a)) - b / np.linalg.norm(b)).max() < 1e-5


@pytest.mark.parametrize('method,nc', [('lgr', None), ('lgr', 250), ('svd', 250), ('svd', None)])
def test_a_pair_alone_equals_the_pair_inside_a_mixed_batch(fx, ops, method, nc):
    """Sizes from 1 to the largest fixture pair in one batch; every record and transform equals the pair's own run, bit for bit."""
    pairs = [constructed_pair(10 + c, c) for c in (1, 2, 63, 257, 1025)] + [pair_of(fx, str(n)) for n in fx['names']]
    order = [5, 0, 9, 1, 6, 2, 10, 3, 7, 4, 8, 11]
    pairs = [pairs[i] for i in order]
    assert max(len(p['corr_scores']) for p in pairs) == 5471
    records, transforms = ops.evaluate_pairs(pairs, method, nc)
    for k, pair in enumerate(pairs):
        rec, T = ops.evaluate_pairs([pair], method, nc)
        assert np.array_equal(rec[0], records[k], equal_nan=True), (k, named(rec[0]), named(records[k]))
        assert np.array_equal(T[0], transforms[k])
        check_against_restatement(records[k], pair, nc, transforms[k], where=f'mixed {k} {method} {nc}')


def empty_meters_as_zero(line):
    """The reference's meters average no records to nan (np.mean of an empty list); Summary prints 0 there."""
    import re
    return re.sub(r'\bnan\b', '0.000', line)


@pytest.mark.parametrize('nc', [0, 250])
def test_cli_reproduces_the_reference_log(fx, tmp_path, capsys, nc):
    from rdmnet_amd import eval as cli
    for name in [str(n) for n in fx['names']]:
        np.savez_compressed(tmp_path / (name + '.npz'), **pair_of(fx, name))
    np.savez_compressed(tmp_path / (str(fx['skipped_name']) + '.npz'), **pair_of(fx, str(fx['names'][0])))
    argv = ['--features-root', str(tmp_path), '--verbose', '--batch', '3', '--workers', '4'] + (['--num_corr', str(nc)] if nc else [])
    cli.main(argv)
    got = capsys.readouterr().out.splitlines()
    want = [empty_meters_as_zero(str(s)) for s in fx[f'lines/lgr/nc{nc}']]
    print('\n'.join(got))
    assert got == want


def test_cli_other_methods_run(fx, tmp_path, capsys):
    from rdmnet_amd import eval as cli
    for name in [str(n) for n in fx['names'][:3]]:
        np.savez_compressed(tmp_path / (name + '.npz'), **pair_of(fx, name))
    for method in ('svd', 'ransac'):
        cli.main(['--features-root', str(tmp_path), '--method', method, '--test_epoch', '3'])
        out = capsys.readouterr().out.splitlines()
        assert out[0] == f'Epoch 3, method {method}' and len(out) == 5 and out[4].startswith('  Registration, RR: ')
