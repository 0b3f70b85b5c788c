"""GPU: the whole forward with top-k attention in the second 3DRoFormer (cfg.thdroformer.k2) against the REFERENCE's own
run (tests/golden/forward_topk_synth0.npz, tests/golden/gen_topk_golden.py: the 15 m crop of synth0, weight seed 0, k2 as
recorded in the file), through the native engine (model(data_dict)) and the per-op mirror; lock-step groups, including
one that mixes k2 and dense engines; and the dense default left exactly as it was.

The judgements are those of test_reference_goldens_gpu.py: float taps within 2e-5 of their maximum, NMS mask equal,
superpoint pairs equal as a set with positions that may differ only inside score ties of 1e-5 (tests/tie_aware.py), point
correspondences equal as a set (at most the rows the reference's own 8- and 1-thread runs differ in), and the pose within
RRE 1e-3 deg / RTE 1e-3 cm of a pose the reference returns from a hypothesis within one inlier of its best."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tie_aware
from sampling import sample

pytestmark = pytest.mark.gpu

OUT_KEYS = ('ref_points_c', 'src_points_c', 'ref_feats_c', 'src_feats_c', 'ref_node_corr_indices', 'src_node_corr_indices',
            'ref_corr_points', 'src_corr_points', 'corr_scores', 'matching_scores', 'estimated_transform')


def npy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


@pytest.fixture(scope='module')
def case(golden_dir):
    from rdmnet_amd import collate, config, model, weights
    g = np.load(os.path.join(golden_dir, 'forward_topk_synth0.npz'))
    cfg = config.make_cfg()
    cfg.thdroformer.k2 = g['k2'].tolist()
    state = weights.synthetic_state_dict(cfg, seed=int(g['weight_seed']))
    net = model.create_model(cfg).cuda()
    net.load_state_dict(state)
    data = collate.collate_pair(g['ref_points_in'], g['src_points_in'], cfg, exact_shapes=True)
    return g, cfg, state, net, data


def test_forward_matches_the_reference(case):
    g, cfg, _, net, data = case
    for i in range(5):
        assert np.array_equal(npy(data['lengths'][i]), g[f'lengths{i}'])
    taps = {}
    out = net(data, taps)  # the per-op mirror
    for k in g.files:
        if k.startswith('tap/encoder.'):
            assert rel(sample(npy(taps[k[4:]])), g[k]) <= 2e-5, k
    for k in ('t1_ref', 't1_src', 't2_ref', 't2_src', 'vote_feats', 'decoder'):
        assert rel(sample(npy(taps[k])), g['tap/' + k]) <= 2e-5, k
    assert rel(npy(taps['vote_xyz']), g['tap/vote_xyz']) <= 1e-6
    assert np.array_equal(npy(taps['nms_mask']).astype(bool), g['tap/nms_mask'])
    for k in ('ref_n2p_scores_c', 'src_n2p_scores_c', 'ref_n2n_scores_c', 'src_n2n_scores_c'):
        assert rel(npy(out[k]), g['out/' + k]) <= 2e-5, k
    for k in ('ref_feats_c', 'src_feats_c', 'ref_feats_f', 'src_feats_f'):
        assert rel(sample(npy(out[k])), g['out/' + k]) <= 2e-5, k
    # superpoint pairs: the same set, a pair elsewhere only inside a group of reference scores tied to 1e-5
    ref_pairs = list(zip(g['out/ref_node_corr_indices'].tolist(), g['out/src_node_corr_indices'].tolist()))
    hip_pairs = list(zip(npy(out['ref_node_corr_indices']).tolist(), npy(out['src_node_corr_indices']).tolist()))
    assert int(g['self/node_corr_symmetric_difference']) == 0
    perm, _ = tie_aware.pair_permutation(hip_pairs, ref_pairs, g['tap/node_corr_scores'].astype(np.float64))
    assert rel(npy(taps['node_corr_scores']), g['tap/node_corr_scores'].astype(np.float64)[perm]) <= 1e-5
    # point correspondences as a set
    hs = tie_aware.corr_rows(npy(out['ref_corr_points']), npy(out['src_corr_points']), npy(out['corr_scores']))
    gs = tie_aware.corr_rows(g['out/ref_corr_points'], g['out/src_corr_points'], g['out/corr_scores'])
    assert len(set(hs) ^ set(gs)) <= int(g['self/corr_symmetric_difference']), (len(hs), len(gs))
    common = sorted(set(hs) & set(gs))
    assert rel([hs[k] for k in common], [gs[k] for k in common]) <= 2e-5
    # pose: one of the reference's poses from the hypotheses within one inlier of its best
    T = npy(out['estimated_transform'])
    errs = [tie_aware.rre_rte(T, A) for A in g['lgr/alt_transforms']]
    assert any(rre <= 1e-3 and rte <= 1e-5 for rre, rte in errs), errs

    # the native engine (model(data_dict)): the per-op path's bits
    nat = net(data)
    for k in OUT_KEYS:
        assert torch.equal(nat[k], out[k]), k


def test_lockstep_groups_are_the_batch_one_bits(case):
    """Four data_dicts (the golden crop and three more crops of the same pair) as one lock-step group equal the batch-1
    calls; then a group of engines that differ in k2 (k2, dense, k2, dense): every pair gets its own configuration's bits."""
    from rdmnet_amd import collate, config, engine
    g, cfg, state, net, data = case
    rp, sp = g['ref_points_in'], g['src_points_in']
    dicts = [data] + [collate.collate_pair(rp[np.linalg.norm(rp[:, :2], axis=1) < r], sp[np.linalg.norm(sp[:, :2], axis=1) < r],
                                           cfg, exact_shapes=True) for r in (14.0, 12.0, 10.0)]
    singles = [{k: v.clone() for k, v in net(d).items() if isinstance(v, torch.Tensor)} for d in dicts]
    group = net(dicts)
    for s, o in zip(singles, group):
        for k in OUT_KEYS:
            assert torch.equal(o[k], s[k]), k

    dense_cfg = config.make_cfg()
    first = engine.Engine(cfg, state)
    engines = [first, engine.Engine(dense_cfg, state, share_with=first), engine.Engine(cfg, state, share_with=first),
               engine.Engine(dense_cfg, state, share_with=first)]
    want = []
    for e, d in zip(engines, dicts):
        e.forward(d)
        want.append((e.transform(), [t.clone() for t in e.corr()]))
    engine.Engine.forward_lockstep(engines, dicts)
    for e, (T, corr) in zip(engines, want):
        assert np.array_equal(e.transform(), T)
        assert all(torch.equal(a, b) for a, b in zip(e.corr(), corr))
    # k2 does change a pair's result: the group above did not run one configuration for all of them
    engines[1].forward(dicts[0])
    assert not torch.equal(engines[1].corr()[2], want[0][1][2])


def test_dense_k2_is_the_default_bits(case):
    """k2 = None (the default, no call into the library) and k2 = [None] * 4 give the same bits as an engine whose top-k
    setting was made and then cleared (rdm_engine_set_attention_topk with n_layers = 0)."""
    from rdmnet_amd import config, engine
    g, cfg, state, _, data = case
    results = []
    for k2 in (None, [None] * 4, 'cleared'):
        c = config.make_cfg()
        if k2 == 'cleared':
            e = engine.Engine(c, state)
            fr = (ctypes.c_double * 4)(0.5, 0.5, 0.5, 0.5)
            assert e.L.rdm_engine_set_attention_topk(e._h, 4, fr) == 0
            assert e.L.rdm_engine_set_attention_topk(e._h, 0, None) == 0
        else:
            c.thdroformer.k2 = k2
            e = engine.Engine(c, state)
        e.keep_taps(True)
        e.forward(data)
        results.append((e.transform(), [t.clone() for t in e.corr()], e.tensor('t2').clone()))
    for T, corr, t2 in results[1:]:
        assert np.array_equal(T, results[0][0])
        assert all(torch.equal(a, b) for a, b in zip(corr, results[0][1]))
        assert torch.equal(t2, results[0][2])
