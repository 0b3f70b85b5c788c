"""Ground-truth superpoint correspondences on the GPU (rdm_gt_node_correspondences, rdm_engine_gt_node_correspondences,
create_eval_model, `python -m rdmnet_amd.infer --gt-nodes`) against the reference's own inputs and outputs
(tests/golden/gt_node_corr.npz: get_node_correspondences as experiments/model.py:283-295 called it, CPU, seeded weights).

Exactness rule: indices torch.equal and overlaps bit-equal; the one allowed difference is a candidate pair whose smallest
point-pair margin |d^2 - r^2| (recorded by the generator) is within 2 fp32 ulp of r^2 -- a tie the reference's own BLAS
could round either way.  The number of such pairs is printed; it is 0 on the committed fixture."""
import ctypes
import glob
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rdmnet_amd import _lib, collate, config, engine, evaluation, model, ops, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, 'golden', 'gt_node_corr.npz')
CASES = ['synth0', 'synth3', 'lowoverlap', 'dense20k', 'scan0_known']
RDM_ERR_CAPACITY = -4


@pytest.fixture(scope='module')
def fx():
    return np.load(FIXTURE)


def _case_clouds(tag):
    """The input clouds of a fixture case (as tests/golden/gen_gt_node_golden.py:case_clouds takes them)."""
    golden = os.path.join(HERE, 'golden')
    if tag == 'scan0_known':
        yaw = np.deg2rad(10.0)
        c, s_ = np.cos(yaw), np.sin(yaw)
        R, t = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]]), np.array([3.0, -1.0, 0.2])
        s0 = np.load(os.path.join(golden, 'scans.npz'))['s000000']
        return s0, ((s0.astype(np.float64) - t) @ R).astype(np.float32)
    f = np.load(os.path.join(golden, f'forward_{tag}.npz'))
    return f['ref_points_in'], f['src_points_in']


_POINTS_F = {}


def fine_points(f, tag):
    """Level 1 of this repository's collate on the case's clouds -- the reference's points_f, checked by its sha256."""
    if tag not in _POINTS_F:
        ref, src = _case_clouds(tag)
        data = collate.collate_pair(ref, src, config.make_cfg(), exact_shapes=True)
        n = int(data['lengths'][1][0])
        pts = data['points'][1].cpu().contiguous()
        halves = (pts[:n].contiguous(), pts[n:].contiguous())
        for side, h in zip(('ref', 'src'), halves):
            assert h.shape[0] == int(f[f'{tag}/n_{side}_points_f']), f'{tag}: {side} fine-point count differs'
            assert hashlib.sha256(h.numpy().tobytes()).hexdigest() == str(f[f'{tag}/{side}_points_f_sha256']), \
                f'{tag}: {side} fine points differ from the reference'
        _POINTS_F[tag] = halves
    return _POINTS_F[tag]


def case_inputs(f, tag, dev='cuda'):
    g = lambda k: torch.from_numpy(np.ascontiguousarray(f[f'{tag}/{k}']))  # noqa: E731
    out = {}
    for side, pts in zip(('ref', 'src'), fine_points(f, tag)):
        idx = g(f'{side}_knn_indices').long()
        padded = torch.cat([pts, torch.zeros_like(pts[:1])])
        out[f'{side}_nodes'] = g(f'{side}_nodes').to(dev)
        out[f'{side}_points'] = pts.to(dev)
        out[f'{side}_idx'] = idx.to(dev)
        out[f'{side}_knn_points'] = padded[idx].to(dev)  # index_select on the padded points (model.py:268-273)
        out[f'{side}_masks'] = g(f'{side}_masks').to(dev)
        out[f'{side}_knn_masks'] = g(f'{side}_knn_masks').to(dev)
    out['transform'] = g('transform').to(dev)
    out['radius'] = float(f[f'{tag}/pos_radius'])
    return out


def gathered(a, transform=None, **masks):
    kw = dict(ref_masks=a['ref_masks'], src_masks=a['src_masks'], ref_knn_masks=a['ref_knn_masks'], src_knn_masks=a['src_knn_masks'])
    kw.update(masks)
    return ops.gt_node_correspondences(a['ref_nodes'], a['src_nodes'], a['ref_knn_points'], a['src_knn_points'],
                                       a['transform'] if transform is None else transform, a['radius'], **kw)


def tie_check(f, tag, idx, ovl, want_idx, want_ovl):
    """Asserts the exactness rule; returns the number of tied candidate pairs (margin within 2 ulp of r^2)."""
    r2 = np.float32(float(f[f'{tag}/pos_radius']) ** 2)
    cand, margin = f[f'{tag}/cand_indices'].astype(np.int64), f[f'{tag}/cand_margin']
    tied = {tuple(p) for p, mg in zip(cand.tolist(), margin) if mg <= 2 * np.spacing(r2)}
    idx, ovl = idx.cpu().numpy(), ovl.cpu().numpy()
    if len(tied) == 0:
        assert np.array_equal(idx, want_idx), f'{tag}: indices differ'
        assert np.array_equal(ovl.view(np.int32), want_ovl.view(np.int32)), f'{tag}: overlaps differ in bits'
        return 0
    got = {tuple(p): o for p, o in zip(idx.tolist(), ovl.view(np.int32).tolist())}
    want = {tuple(p): o for p, o in zip(want_idx.tolist(), want_ovl.view(np.int32).tolist())}
    bad = [p for p in set(got) | set(want) if got.get(p) != want.get(p) and p not in tied]
    assert not bad, f'{tag}: {len(bad)} pairs differ outside ties, e.g. {bad[:5]}'
    return len(tied)


@pytest.mark.parametrize('tag', CASES)
def test_op_equals_reference_on_its_own_inputs(fx, tag):
    a = case_inputs(fx, tag)
    idx, ovl = gathered(a)
    n_tied = tie_check(fx, tag, idx, ovl, fx[f'{tag}/corr_indices'], fx[f'{tag}/corr_overlaps'])
    # the indexed form (point_to_node's layout, what the engine holds) gives the same, and B is the reference's
    idx2, ovl2, B = ops.gt_node_correspondences_indexed(a['ref_nodes'], a['src_nodes'], a['ref_points'], a['ref_idx'], a['src_points'],
                                                        a['src_idx'], a['transform'], a['radius'], a['ref_masks'], a['src_masks'],
                                                        a['ref_knn_masks'], a['src_knn_masks'])
    assert torch.equal(idx2, idx) and torch.equal(ovl2.view(torch.int32), ovl.view(torch.int32))
    assert B == int(fx[f'{tag}/B'])
    assert idx.dtype == torch.int64 and ovl.dtype == torch.float32 and idx.shape == (ovl.shape[0], 2)
    m, n = a['ref_nodes'].shape[0], a['src_nodes'].shape[0]
    print(f'{tag}: M={m} N={n} M*N={m * n} B={B} C={idx.shape[0]} tied candidate pairs (margin <= 2 ulp of r^2): {n_tied}')
    if tag == 'dense20k':
        assert m * n > 2 ** 16


def test_far_transform_gives_no_correspondences(fx):
    a = case_inputs(fx, 'synth0')
    T = a['transform'].clone()
    T[0, 3] += 1000.0  # src 1 km away
    idx, ovl = gathered(a, transform=T)
    assert idx.shape == (0, 2) and ovl.shape == (0,) and idx.dtype == torch.int64


def test_all_masked_nodes_give_no_correspondences(fx):
    a = case_inputs(fx, 'synth0')
    for which in ('ref_masks', 'src_masks'):
        idx, ovl = gathered(a, **{which: torch.zeros_like(a[which])})
        assert idx.shape == (0, 2) and ovl.shape == (0,)


def test_default_masks_are_all_valid(fx):
    a = case_inputs(fx, 'synth0')
    ones = dict(ref_masks=torch.ones_like(a['ref_masks']), src_masks=torch.ones_like(a['src_masks']),
                ref_knn_masks=torch.ones_like(a['ref_knn_masks']), src_knn_masks=torch.ones_like(a['src_knn_masks']))
    i1, o1 = gathered(a, **ones)
    i2, o2 = ops.gt_node_correspondences(a['ref_nodes'], a['src_nodes'], a['ref_knn_points'], a['src_knn_points'], a['transform'],
                                         a['radius'])
    assert torch.equal(i1, i2) and torch.equal(o1, o2)


def test_single_valid_slot_patches(fx):
    """Every patch keeps only its nearest point: a pair matches iff those two points lie within r (the sphere test passes
    whenever they do), and its overlap is then exactly (1/1 + 1/1) / 2 = 1."""
    a = case_inputs(fx, 'synth0')
    km = {k: torch.zeros_like(a[k]) for k in ('ref_knn_masks', 'src_knn_masks')}
    for k in km:
        km[k][:, 0] = a[k][:, 0]
    idx, ovl = gathered(a, **km)
    assert idx.shape[0] > 0 and bool((ovl == 1.0).all())
    T = a['transform'].double().cpu()
    p = a['ref_knn_points'][:, 0].double().cpu()
    q = a['src_knn_points'][:, 0].double().cpu() @ T[:3, :3].T + T[:3, 3]
    d2 = ((p[:, None] - q[None]) ** 2).sum(-1)
    valid = (a['ref_masks'] & km['ref_knn_masks'][:, 0]).cpu()[:, None] & (a['src_masks'] & km['src_knn_masks'][:, 0]).cpu()[None]
    r2 = a['radius'] ** 2
    want = set(map(tuple, torch.nonzero(valid & (d2 < r2)).tolist()))
    near = set(map(tuple, torch.nonzero(valid & ((d2 - r2).abs() < 1e-5)).tolist()))
    got = set(map(tuple, idx.cpu().tolist()))
    assert not ((got ^ want) - near), sorted((got ^ want) - near)[:5]


def _raw_call(a, out_idx, out_ovl, capacity, counts):
    L = _lib.lib()
    m, n, k = a['ref_nodes'].shape[0], a['src_nodes'].shape[0], a['ref_idx'].shape[1]
    ws = torch.empty(L.rdm_gt_node_correspondences_workspace_bytes(m, n), dtype=torch.uint8, device='cuda')
    masks = [a[x].view(torch.uint8) if a[x].dtype == torch.bool else a[x] for x in ('ref_masks', 'src_masks', 'ref_knn_masks', 'src_knn_masks')]
    return L.rdm_gt_node_correspondences(
        a['ref_nodes'].data_ptr(), m, a['src_nodes'].data_ptr(), n, a['ref_points'].data_ptr(), a['ref_idx'].data_ptr(),
        a['ref_points'].shape[0], a['src_points'].data_ptr(), a['src_idx'].data_ptr(), a['src_points'].shape[0], k,
        *[t.data_ptr() for t in masks], a['transform'].data_ptr(), a['radius'], out_idx.data_ptr(), out_ovl.data_ptr(), capacity,
        counts.data_ptr(), counts[2:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr())


def test_small_capacity_reports_and_stays_in_bounds(fx):
    a = case_inputs(fx, 'synth0')
    C = fx['synth0/corr_indices'].shape[0]
    cap, guard = C - 7, 64
    out_idx = torch.full(((cap + guard) * 2,), -12345, dtype=torch.int64, device='cuda')
    out_ovl = torch.full((cap + guard,), -3.0, dtype=torch.float32, device='cuda')
    counts = torch.zeros(3, dtype=torch.int32, device='cuda')
    assert _raw_call(a, out_idx, out_ovl, cap, counts) == 0
    c, b, status = counts.cpu().tolist()
    assert (c, b, status) == (C, int(fx['synth0/B']), 1)  # status != 0 = RDM_ERR_CAPACITY for the caller
    assert bool((out_idx[2 * cap:] == -12345).all()) and bool((out_ovl[cap:] == -3.0).all()), 'wrote past capacity'
    assert np.array_equal(out_idx[:2 * cap].view(cap, 2).cpu().numpy(), fx['synth0/corr_indices'][:cap])


def _synth_pair(i):
    s = np.load(os.path.join(HERE, 'golden', 'synthetic_pairs.npz'))
    return s[f'ref{i}'], s[f'src{i}'], s[f'T{i}'].astype(np.float32)


@pytest.fixture(scope='module')
def state():
    return weights.synthetic_state_dict(config.make_cfg(), seed=0)


def test_engine_entry_equals_the_op_on_the_runs_exported_tensors(state):
    cfg = config.make_cfg()
    ref, src, T = _synth_pair(0)
    eng = engine.Engine(cfg, state)
    eng.keep_taps(True)
    res = eng.run(torch.from_numpy(ref).cuda(), torch.from_numpy(src).cuda())
    idx, ovl, B = eng.gt_node_correspondences(T, 0.6)
    m_r, nf_r = int(res.n_ref_nodes), int(res.level_ref_sizes[1])
    t = {k: eng.tensor(k) for k in ('nodes', 'points1', 'ref_knn', 'src_knn', 'ref_knn_masks', 'src_knn_masks', 'ref_node_masks',
                                    'src_node_masks')}
    nodes, pf = t['nodes'].contiguous(), t['points1'].contiguous()
    want = ops.gt_node_correspondences_indexed(nodes[:m_r], nodes[m_r:], pf[:nf_r], t['ref_knn'].contiguous(), pf[nf_r:],
                                               t['src_knn'].contiguous(), torch.from_numpy(T).cuda(), 0.6,
                                               t['ref_node_masks'][:, 0].contiguous(), t['src_node_masks'][:, 0].contiguous(),
                                               t['ref_knn_masks'].contiguous(), t['src_knn_masks'].contiguous())
    assert torch.equal(idx, want[0]) and torch.equal(ovl.view(torch.int32), want[1].view(torch.int32)) and B == want[2]
    assert idx.shape[0] > 0
    # capacity too small: the capacity error, nothing past it
    L = _lib.lib()
    cap, guard = idx.shape[0] - 3, 32
    out_idx = torch.full(((cap + guard) * 2,), -7, dtype=torch.int64, device='cuda')
    out_ovl = torch.full((cap + guard,), -1.0, dtype=torch.float32, device='cuda')
    counts = (ctypes.c_int64 * 2)()
    Td = torch.from_numpy(T).cuda()
    rc = L.rdm_engine_gt_node_correspondences(eng._h, Td.data_ptr(), 0.6, out_idx.data_ptr(), out_ovl.data_ptr(), cap, counts,
                                              _lib.stream_ptr())
    assert rc == RDM_ERR_CAPACITY and counts[0] == idx.shape[0] and counts[1] == B
    assert bool((out_idx[2 * cap:] == -7).all()) and bool((out_ovl[cap:] == -1.0).all())
    assert torch.equal(out_idx[:2 * cap].view(cap, 2), idx[:cap])


def test_engine_entry_without_a_forward_fails_clearly(state):
    cfg = config.make_cfg()
    eng = engine.Engine(cfg, state)
    with pytest.raises(RuntimeError, match='no completed forward run'):
        eng.gt_node_correspondences(np.eye(4, dtype=np.float32))
    ref, src, _ = _synth_pair(0)
    eng.collate(torch.from_numpy(ref).cuda(), torch.from_numpy(src).cuda())  # a collate alone is not a forward
    with pytest.raises(RuntimeError, match='no completed forward run'):
        eng.gt_node_correspondences(np.eye(4, dtype=np.float32))


def test_op_rejects_bad_arguments(fx):
    a = case_inputs(fx, 'synth0')
    with pytest.raises(RuntimeError, match='dtype'):
        ops.gt_node_correspondences(a['ref_nodes'].double(), a['src_nodes'], a['ref_knn_points'], a['src_knn_points'], a['transform'], 0.6)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.gt_node_correspondences(a['ref_nodes'].cpu(), a['src_nodes'], a['ref_knn_points'], a['src_knn_points'], a['transform'], 0.6)
    with pytest.raises(RuntimeError, match='on cpu'):
        ops.gt_node_correspondences(a['ref_nodes'], a['src_nodes'].cpu(), a['ref_knn_points'], a['src_knn_points'], a['transform'], 0.6)
    with pytest.raises(RuntimeError, match='shape'):
        ops.gt_node_correspondences(a['ref_nodes'], a['src_nodes'], a['ref_knn_points'], a['src_knn_points'][:-1], a['transform'], 0.6)
    with pytest.raises(RuntimeError, match='shape'):
        ops.gt_node_correspondences(a['ref_nodes'], a['src_nodes'], a['ref_knn_points'], a['src_knn_points'], a['transform'][:3], 0.6)


def test_eval_model_adds_the_two_keys_to_create_models_outputs(fx, state):
    cfg = config.make_cfg()
    ref, src, T = _synth_pair(0)
    assert np.array_equal(T, fx['e2e/transform'])
    net = model.create_model(cfg).cuda()
    net.load_state_dict(state)
    ev = model.create_eval_model(cfg).cuda()
    ev.load_state_dict(state)
    dd = collate.collate_pair(ref, src, cfg, exact_shapes=True)
    out = net(dd)
    dd['transform'] = torch.from_numpy(T).cuda()
    eout = ev(dd)
    assert len(out) == 31 and set(eout) == set(out) | {'gt_node_corr_indices', 'gt_node_corr_overlaps'}
    for k, v in out.items():
        assert torch.equal(eout[k], v), k
    dev = max(float((eout['ref_points_c'].cpu() - torch.from_numpy(fx['e2e/ref_points_c'])).abs().max()),
              float((eout['src_points_c'].cpu() - torch.from_numpy(fx['e2e/src_points_c'])).abs().max()))
    n_tied = tie_check(fx, 'synth0', eout['gt_node_corr_indices'], eout['gt_node_corr_overlaps'], fx['e2e/gt_node_corr_indices'],
                       fx['e2e/gt_node_corr_overlaps'])
    print(f'end to end: C={eout["gt_node_corr_indices"].shape[0]}, superpoints vs the reference max |d| {dev:.2e}, tied pairs {n_tied}')
    # the per-op mirror (taps) gives the same two keys
    tout = ev(dd, {})
    assert torch.equal(tout['gt_node_corr_indices'], eout['gt_node_corr_indices'])
    assert torch.equal(tout['gt_node_corr_overlaps'], eout['gt_node_corr_overlaps'])


def test_infer_gt_nodes_writes_test_py_files_and_real_coarse_meters(tmp_path):
    out_dir = tmp_path / 'out'
    cmd = [sys.executable, '-m', 'rdmnet_amd.infer', '--synthetic', '8', '--synthetic-distinct', '2', '--synthetic-cache',
           str(tmp_path / 'pairs'), '--gt-nodes', '--out', str(out_dir), '--quiet']
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    files = sorted(glob.glob(str(out_dir / '*.npz')))
    assert files
    want_keys = set(evaluation.TEST_NPZ_KEYS) | {'transform'}
    precisions = []
    for fn in files:
        d = np.load(fn)
        assert set(d.files) == want_keys, fn
        precisions.append(evaluation.evaluate_sparse_correspondences(d['ref_points_c'], d['src_points_c'], d['ref_node_corr_indices'],
                                                                     d['src_node_corr_indices'], d['gt_node_corr_indices'])['precision'])
        assert d['gt_node_corr_indices'].shape[0] > 0
    # the 8 pairs cycle through 2 distinct ones: the same file names are rewritten, the meters see all 8 pairs
    line = [x for x in p.stdout.splitlines() if 'Coarse Matching' in x][0]
    got = [float(v) for v in re.findall(r':\s*([0-9.]+)', line)]
    pr = np.asarray(precisions * (8 // len(precisions)))
    want = [pr.mean(), (pr > 0).mean(), (pr >= 0.1).mean(), (pr >= 0.3).mean(), (pr >= 0.5).mean()]
    assert [f'{v:.3f}' for v in got] == [f'{v:.3f}' for v in want], (line, want)
    print(line)
