"""GPU: cfg.fine_matching's options on the device -- rdm_lgr_options teacher-forced on the LGR inputs of the goldens against
the reference's LocalGlobalRegistration (tests/golden/lgr_options.npz, gen_lgr_options_golden.py), the general extraction kernel
against the specialised one, constructed ties against tests/lgr_options_restatement.py, and the engine with options against
the operator mirror, alone and in lock-step groups."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lgr_options_restatement as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ENTRIES = R.fixture_entries(GOLDEN)
EPS32 = float(np.finfo(np.float32).eps)


def device_inputs(inputs):
    rp, sp, rm, sm, ms, gs = inputs
    return (ms.cuda().contiguous(), rp.cuda().contiguous(), sp.cuda().contiguous(), rm.to(torch.uint8).cuda().contiguous(),
            sm.to(torch.uint8).cuda().contiguous(), gs.cuda().contiguous())


def gpu_lgr(inputs, fm, opt):
    """ops.lgr on CPU inputs -> (ref rows, src rows, scores, T, counts) as numpy, the C valid rows only."""
    from rdmnet_amd import ops
    ms, rp, sp, rm, sm, gs = device_inputs(inputs)
    rc, sc, cs, T, counts = ops.lgr(ms, rp, sp, rm, sm, fm.acceptance_radius, fm.correspondence_threshold, fm.num_refinement_steps,
                                    global_scores=gs, **opt)
    counts = counts.cpu().numpy()
    C = int(counts[0])
    assert 0 <= C <= rc.shape[0]
    return rc[:C].cpu().numpy(), sc[:C].cpu().numpy(), cs[:C].cpu().numpy(), T.cpu().numpy(), counts


def triples_of(rc, sc, candidates, rp, sp):
    """The (patch, i, j) of every output row: outputs and `candidates` (sorted triples) are both in nonzero order, so the rows
    are matched to the candidates front to back by their points; a row that matches no remaining candidate fails."""
    rp, sp = rp.numpy(), sp.numpy()
    out, c = [], 0
    for r in range(len(rc)):
        while c < len(candidates) and not (np.array_equal(rp[candidates[c][0], candidates[c][1]], rc[r]) and
                                           np.array_equal(sp[candidates[c][0], candidates[c][2]], sc[r])):
            c += 1
        assert c < len(candidates), f'output row {r} is no correspondence the reference lists or leaves undecided'
        out.append(candidates[c])
        c += 1
    return out


def check_pose(T, counts, ref_v, src_v, w_v, f, fm, full_size):
    """The LGR pose bounds of test_reference_goldens_gpu.py: 1e-3 deg and 1e-5 m (1e-4 m at full size) against the float64
    Procrustes of the same verification set and final inliers, and against the reference's fp32 pose of the same hypothesis
    unless that covariance is rank-deficient (sigma2 / sigma1 <= 1e-3, as test_harness_gpu.py).
    The float64 solution takes its inliers from the RETURNED pose, the kernel's last step from the pose before it: the two
    sets are the same once the refinement has converged, which holds when no residual lies within 1e-4 m of the radius (ten
    times the translation bound: a step of a converged refinement moves no point further) -- asserted, as
    test_full_size_configs_gpu.py does."""
    from oracle import forward as ofw
    bound_t = 1e-4 if full_size else 1e-5
    alts = f['alt_hypotheses'].tolist()
    assert int(counts[2]) in alts, (int(counts[2]), alts)  # within one inlier of the reference's best (tie_aware.py)
    if 'inlier_counts' in f:
        assert int(counts[1]) == len(f['inlier_counts'])
    inl, edge = R.final_inliers(T, ref_v, src_v, fm.acceptance_radius)
    T64, S = ofw.procrustes_fp64(src_v, ref_v, np.asarray(w_v, np.float64) * inl)
    e64 = ofw.rre_rte(T, T64)
    ref_T = f['transform'] if ('best' not in f or int(counts[2]) == int(f['best'])) else f['alt_transforms'][alts.index(int(counts[2]))]
    eref = ofw.rre_rte(T, ref_T)
    ratio = S[1] / S[0] if S[0] > 0 else 1.0  # (no inlier left: a zero covariance, whose torch.svd pose is exactly the identity)
    print(f'  pose: vs float64 rre {e64[0]:.2e} deg rte {e64[1]:.2e} m; vs reference rre {eref[0]:.2e} deg rte {eref[1]:.2e} m; '
          f'sigma2/sigma1 {ratio:.2e}; inliers {int(inl.sum())}/{len(inl)}; nearest residual to the radius {edge:.2e} m')
    assert edge > 1e-4, edge  # no inlier decision on the edge
    assert e64[0] <= 1e-3 and e64[1] <= bound_t, e64
    if ratio > 1e-3:
        assert eref[0] <= 1e-3 and eref[1] <= bound_t, eref


@pytest.mark.parametrize('case,name', ENTRIES)
def test_lgr_options_reproduces_the_reference_teacher_forced(case, name):
    """Correspondences by the fixture's rule (exact cases: the reference's triples in its order; synth0: every decided entry
    as the reference decided, at most 2 % undecided), corr_scores to 2 ulp (one exp and at most one multiply), the chosen
    hypothesis within the reference's near-tied ones, the pose as check_pose says.  synth0/set4_nolimit refines 5 471
    correspondences: the path of the refinement that reads global memory instead of its LDS stage (> 4 608)."""
    from rdmnet_amd import config
    opt, f = R.fixture_entry(GOLDEN, case, name)
    inputs = R.golden_inputs(GOLDEN, case)
    fm = config.make_cfg().fine_matching
    rc, sc, cs, T, counts = gpu_lgr(inputs, fm, opt)
    want = [tuple(r) for r in f['indices'].astype(np.int64).tolist()]
    cand = sorted(set(want) | {tuple(r) for r in f['undecided'].astype(np.int64).tolist()})
    got = triples_of(rc, sc, cand, inputs[0], inputs[1])
    differ = R.compare_correspondences(np.asarray(got, np.int64).reshape(-1, 3), f)
    ws = dict(zip(want, f['corr_scores'].astype(np.float64).tolist()))
    rel = max((abs(float(s) - ws[t]) / ws[t] for t, s in zip(got, cs) if t in ws), default=0.0)
    print(f'{case}/{name}: C {len(got)} (reference {len(want)}, {differ} differ inside the undecided set), corr_scores rel {rel:.2e}, '
          f'hypotheses {int(counts[1])}, best {int(counts[2])}')
    assert rel <= 2 * EPS32, rel
    if name == 'set4_nolimit':
        assert len(got) > 4608
    ver = R.verification_set(torch.from_numpy(cs), opt['correspondence_limit']).numpy()
    check_pose(T, counts, rc[ver], sc[ver], cs[ver], f, fm, full_size=case not in ('small', 'crop9'))


@pytest.mark.parametrize('case', ['crop9', 'synth3'])
def test_default_options_through_the_general_kernel_equal_rdm_lgr(case):
    """rdm_lgr_options with the shipped values runs the general extraction kernel; everything it returns equals rdm_lgr's."""
    from rdmnet_amd import _lib, config, ops
    L = _lib.lib()
    fm = config.make_cfg().fine_matching
    ms, rp, sp, rm, sm, gs = device_inputs(R.golden_inputs(GOLDEN, case))
    b, side = rm.shape
    want = ops.lgr(ms, rp, sp, rm, sm, fm.acceptance_radius, fm.correspondence_threshold, fm.num_refinement_steps)
    opt = _lib.FineMatchingOptions.of()
    cap = L.rdm_lgr_options_capacity(b, side, ctypes.byref(opt))
    assert cap == want[0].shape[0]
    rc, sc = torch.empty((cap, 3), device='cuda'), torch.empty((cap, 3), device='cuda')
    cs, T, counts = torch.empty((cap,), device='cuda'), torch.empty((4, 4), device='cuda'), torch.empty((3,), dtype=torch.int32, device='cuda')
    ws = ops.scratch(ms.device, L.rdm_lgr_options_workspace_bytes(b, side, ctypes.byref(opt)))
    _lib.check(L.rdm_lgr_options(ms.data_ptr(), side + 1, rp.data_ptr(), sp.data_ptr(), rm.data_ptr(), sm.data_ptr(), 0, b, side,
                                 fm.acceptance_radius, fm.correspondence_threshold, fm.num_refinement_steps, ctypes.byref(opt),
                                 rc.data_ptr(), sc.data_ptr(), cs.data_ptr(), T.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _lib.stream_ptr()), 'rdm_lgr_options')
    C = int(want[4][0])
    assert C > 0 and torch.equal(counts, want[4]) and torch.equal(T, want[3])
    assert torch.equal(rc[:C], want[0][:C]) and torch.equal(sc[:C], want[1][:C]) and torch.equal(cs[:C], want[2][:C])


def test_invalid_options_are_rejected_by_ops_and_by_the_library():
    """ops.lgr raises a ValueError naming the argument (nothing is truncated to an int); the C entry returns an error."""
    from rdmnet_amd import _lib, config, ops
    L = _lib.lib()
    fm = config.make_cfg().fine_matching
    ms, rp, sp, rm, sm, gs = device_inputs(R.golden_inputs(GOLDEN, 'small'))
    b, side = rm.shape
    for key, bad in (('topk', dict(topk=0)), ('topk', dict(topk=130)), ('topk', dict(topk=129, use_dustbin=False)),
                     ('topk', dict(topk=2.5)), ('confidence_threshold', dict(confidence_threshold=-0.1, use_dustbin=False)),
                     ('correspondence_limit', dict(correspondence_limit=-2)), ('correspondence_limit', dict(correspondence_limit=7.9)),
                     ('mutual', dict(mutual=1)), ('global_scores', dict(use_global_score=True))):
        with pytest.raises(ValueError, match=key):
            ops.lgr(ms, rp, sp, rm, sm, fm.acceptance_radius, fm.correspondence_threshold, fm.num_refinement_steps, **bad)
    out = torch.empty((b * 2 * side, 3), device='cuda')
    for bad in (_lib.FineMatchingOptions.of(topk=0), _lib.FineMatchingOptions.of(topk=130), _lib.FineMatchingOptions.of(confidence_threshold=-1.0),
                _lib.FineMatchingOptions.of(correspondence_limit=-1), _lib.FineMatchingOptions.of(use_global_score=True)):
        rc = L.rdm_lgr_options(ms.data_ptr(), side + 1, rp.data_ptr(), sp.data_ptr(), rm.data_ptr(), sm.data_ptr(), 0, b, side,
                               fm.acceptance_radius, fm.correspondence_threshold, fm.num_refinement_steps, ctypes.byref(bad),
                               out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), 1 << 20,
                               _lib.stream_ptr())
        assert rc != 0 and L.rdm_last_error()


def quantised_patches(seed, batch=3, side=64, levels=6):
    """Patches whose scores take a handful of values, so that every k-th boundary and the limit sit inside groups of exactly
    equal scores; masked lines hold the Sinkhorn fill."""
    rng = np.random.default_rng(seed)
    vals = np.log(np.linspace(0.02, 0.4, levels)).astype(np.float32)
    L = vals[rng.integers(0, levels, size=(batch, side + 1, side + 1))]
    rm, sm = rng.random((batch, side)) < 0.8, rng.random((batch, side)) < 0.7
    rm[0, :], sm[0, :] = True, True  # one patch without a masked line
    for b in range(batch):
        L[b, :side][~rm[b]] = np.float32(-1e12)
        L[b, :, :side][:, ~sm[b]] = np.float32(-1e12)
    pts = lambda: torch.from_numpy(rng.normal(size=(batch, side, 3)).astype(np.float32) * 5)
    return pts(), pts(), torch.from_numpy(rm), torch.from_numpy(sm), torch.from_numpy(L), torch.from_numpy(rng.random(batch).astype(np.float32))


def test_the_constructed_tie_patch_keeps_the_lowest_index():
    """The patch of lgr_options_restatement.tie_patch: exact ties at the k-th boundary of a row and of a column, mutual."""
    from rdmnet_amd import config
    fm = config.make_cfg().fine_matching
    inputs, opt = R.tie_patch(), R.options(topk=2, mutual=True)
    want = R.lgr(*inputs, fm, opt)
    rc, sc, cs, T, counts = gpu_lgr(inputs, fm, opt)
    assert len(cs) == len(want['corr_scores']) > 0
    assert np.array_equal(rc, want['ref_corr_points'].numpy()) and np.array_equal(sc, want['src_corr_points'].numpy())
    assert np.allclose(cs, want['corr_scores'].numpy(), rtol=2 * EPS32, atol=0)


@pytest.mark.parametrize('k', [1, 2, 5, 32, 33, 40, 64, 65])
@pytest.mark.parametrize('mutual,dustbin,limit', [(False, True, None), (True, False, None), (False, False, 40), (True, True, 7)])
def test_ties_at_every_boundary_match_the_restatement(k, mutual, dustbin, limit):
    """Lowest-index rule of the top-k on patches full of exact ties, for k from 1 up to the line length (64, 65 with the
    dustbin; k = 65 without it runs as 64): the same correspondences in the same order as the restatement, scores to 2 ulp,
    the same number of hypotheses, with and without a limit.  (Which correspondences a limit keeps among tied scores is the
    subject of test_the_limit_keeps_the_lowest_positions_among_tied_scores.)"""
    from rdmnet_amd import config
    fm = config.make_cfg().fine_matching
    opt = R.options(topk=min(k, 64 + (1 if dustbin else 0)), mutual=mutual, use_dustbin=dustbin, confidence_threshold=0.05,
                    use_global_score=True, correspondence_limit=limit)
    inputs = quantised_patches(seed=k)
    want = R.lgr(*inputs, fm, opt)
    rc, sc, cs, T, counts = gpu_lgr(inputs, fm, opt)
    assert len(cs) == len(want['corr_scores']) > (limit or 0)
    assert np.array_equal(rc, want['ref_corr_points'].numpy()) and np.array_equal(sc, want['src_corr_points'].numpy())
    assert np.allclose(cs, want['corr_scores'].numpy(), rtol=2 * EPS32, atol=0)
    assert int(counts[1]) == len(want['chunks']) and np.isfinite(T).all()


def rigid(axis, deg, t):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = t
    return T


def limit_tie_scene(n_patches, side=8, seed=0):
    """Patches whose only correspondences are their diagonals (k = 1, dustbin), every third patch with score 0.3, the others
    0.2: with L = (all of the 0.3) + need the L-th score sits inside the group of EQUAL 0.2 scores, 1 < need < their number,
    and need splits a patch.  The correspondences the lowest-position rule keeps follow one rigid motion T1 up to 0.1 m of
    noise, so the weighted least-squares pose depends on exactly which rows are in the verification set; every other
    correspondence follows T2, 100+ degrees and tens of metres away -- the pose a rule keeping other tied positions ends at.
    -> (LGR inputs, options, T1, T2, kept positions)."""
    rng = np.random.default_rng(seed)
    a, hi, z, d = (np.float32(np.log(v)) for v in (0.2, 0.3, 0.001, 0.05))
    L = np.full((n_patches, side + 1, side + 1), z, np.float32)
    L[:, :side, side], L[:, side, :side] = d, d
    high = np.arange(n_patches) % 3 == 1
    for p in range(n_patches):
        L[p, np.arange(side), np.arange(side)] = hi if high[p] else a
    n_tied = int((~high).sum()) * side
    need = n_tied // 2 + 3
    limit = int(high.sum()) * side + need
    scores = np.repeat(np.where(high, np.float32(0.3), np.float32(0.2)), side)  # nonzero order: position = patch * side + i
    kept = np.zeros(n_patches * side, bool)
    kept[R.verification_set(torch.from_numpy(scores), limit).numpy()] = True
    assert kept.sum() == limit and 1 < need < n_tied and need % side != 0
    T1, T2 = rigid([0.2, -0.3, 1.0], 30.0, [1.0, 2.0, 0.5]), rigid([1.0, 0.4, -0.2], -100.0, [30.0, -20.0, 10.0])
    ref = rng.normal(size=(n_patches * side, 3)) * 5
    src1 = (ref - T1[:3, 3]) @ T1[:3, :3] + rng.normal(size=ref.shape) * 0.1  # ref = R1 src + t1 (+ noise)
    src2 = (ref - T2[:3, 3]) @ T2[:3, :3]
    src = np.where(kept[:, None], src1, src2)
    inputs = (torch.from_numpy(ref.astype(np.float32).reshape(n_patches, side, 3)), torch.from_numpy(src.astype(np.float32).reshape(n_patches, side, 3)),
              torch.ones(n_patches, side, dtype=torch.bool), torch.ones(n_patches, side, dtype=torch.bool), torch.from_numpy(L),
              torch.ones(n_patches))
    return inputs, R.options(correspondence_limit=limit), T1, T2, np.nonzero(kept)[0]


@pytest.mark.parametrize('n_patches', [6, 160])
def test_the_limit_keeps_the_lowest_positions_among_tied_scores(n_patches):
    """The device's verification set when the L-th score is tied (limit_tie_scene; 160 patches: 1 280 correspondences, more than
    one 1 024-thread pass of the selection).  What the kernel kept is read off its results: the chosen hypothesis is within one
    inlier of the restatement's best, and the pose equals -- 1e-3 deg, 1e-5 m -- the float64 weighted Procrustes of exactly the
    restatement's verification rows (all of them inliers; a row more, less or other moves that solution by 0.1 m / n, above
    the bound) and lies next to T1, not T2."""
    from oracle import forward as ofw
    from rdmnet_amd import config
    fm = config.make_cfg().fine_matching
    inputs, opt, T1, T2, kept = limit_tie_scene(n_patches)
    want = R.lgr(*inputs, fm, opt)
    assert np.array_equal(want['verification'].numpy(), kept)
    rc, sc, cs, T, counts = gpu_lgr(inputs, fm, opt)
    assert len(cs) == n_patches * 8 > opt['correspondence_limit'] and int(counts[0]) == len(cs)
    assert np.array_equal(rc, want['ref_corr_points'].numpy()) and np.array_equal(sc, want['src_corr_points'].numpy())
    assert int(counts[1]) == n_patches == len(want['chunks'])
    wc = want['inlier_counts'].numpy()
    assert wc.max() == len(kept) and int(counts[2]) in np.nonzero(wc >= wc.max() - 1)[0].tolist(), (int(counts[2]), wc)
    inl, edge = R.final_inliers(T, rc[kept], sc[kept], fm.acceptance_radius)
    assert inl.all() and edge > 1e-4
    T64, _ = ofw.procrustes_fp64(sc[kept], rc[kept], cs[kept].astype(np.float64))
    rre, rte = ofw.rre_rte(T, T64)
    print(f'limit ties, {n_patches} patches: kept {len(kept)} of {len(cs)}, best {int(counts[2])}, pose vs float64 of the kept rows '
          f'rre {rre:.2e} deg rte {rte:.2e} m; vs T1 {ofw.rre_rte(T, T1)}, vs T2 {ofw.rre_rte(T, T2)}')
    assert rre <= 1e-3 and rte <= 1e-5, (rre, rte)
    other = np.setdiff1d(np.arange(len(cs)), kept)[-len(kept):] if len(cs) - len(kept) >= len(kept) else None
    if other is not None:  # (the float64 solution of another choice among the ties is far away: the comparison above can tell)
        assert ofw.rre_rte(ofw.procrustes_fp64(sc[other], rc[other], cs[other].astype(np.float64))[0], T64)[0] > 1.0
    assert ofw.rre_rte(T, T1)[0] < 1.0 and ofw.rre_rte(T, T2)[0] > 50.0


def test_a_refinement_without_inliers_returns_the_identity_on_the_shipped_path():
    """rdm_lgr (shipped options): one patch whose correspondences follow no rigid motion -- its hypothesis has no inlier, the
    refinement's covariance is zero, and the pose is the identity, as the reference's torch.svd of a zero matrix gives
    (oracle.forward.lgr)."""
    from oracle import forward as ofw
    from rdmnet_amd import config
    cfg = config.make_cfg()
    rng = np.random.default_rng(3)
    side = 4
    L = np.full((1, side + 1, side + 1), np.float32(np.log(0.001)), np.float32)
    L[0, np.arange(side), np.arange(side)] = np.float32(np.log(0.3))
    L[0, :side, side], L[0, side, :side] = np.float32(np.log(0.05)), np.float32(np.log(0.05))
    pts = lambda: torch.from_numpy((rng.normal(size=(1, side, 3)) * 100).astype(np.float32))
    inputs = (pts(), pts(), torch.ones(1, side, dtype=torch.bool), torch.ones(1, side, dtype=torch.bool), torch.from_numpy(L), torch.ones(1))
    orc, osc, ocs, oT, info = ofw.lgr(inputs[0], inputs[1], inputs[2], inputs[3], inputs[4], cfg)
    assert int(info['inlier_counts'].max()) == 0 and np.array_equal(oT.numpy(), np.eye(4, dtype=np.float32))
    rc, sc, cs, T, counts = gpu_lgr(inputs, cfg.fine_matching, R.options())
    assert len(cs) == side and int(counts[1]) == 1 and np.array_equal(T, np.eye(4, dtype=np.float32)), T


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope='module')
def scene(oracle_native, golden_dir):
    from rdmnet_amd import collate, config, weights
    cfg = config.make_cfg()
    z = np.load(os.path.join(golden_dir, 'synthetic_pairs.npz'))
    g = np.load(os.path.join(golden_dir, 'forward_small.npz'))
    return dict(state=weights.synthetic_state_dict(cfg, seed=0), collate=collate,
                clouds=[(g['ref_points_in'], g['src_points_in']), (z['ref0'], z['src0'])])


def make_net(scene, **fine_matching):
    from rdmnet_amd import config, model
    cfg = config.make_cfg()
    cfg.fine_matching.update(fine_matching)
    net = model.create_model(cfg).cuda()
    net.load_state_dict(scene['state'])
    return cfg, net


OPTION_SETS = {'limit': dict(topk=3, use_dustbin=False, confidence_threshold=0.05, use_global_score=True, correspondence_limit=300),
               'mutual': dict(topk=2, mutual=True)}


@pytest.mark.parametrize('which', sorted(OPTION_SETS))
def test_engine_with_options_equals_the_operator_mirror_alone_and_in_lock_step(scene, which):
    """create_model(cfg)(data_dict) -- one native call -- equals the operator mirror of model.py key by key; a lock-step group
    gives every pair the output of its batch-1 call; the options change the result (they are not ignored)."""
    cfg, net = make_net(scene, **OPTION_SETS[which])
    _, plain = make_net(scene)
    with torch.cuda.stream(torch.cuda.Stream()):
        dicts = [scene['collate'].collate_pair(r, s, cfg) for r, s in scene['clouds']]
        want = []
        for d in dicts:
            out, mirror = net(d), net(d, {})
            assert set(out) == set(mirror) and len(out) == 31
            for key in out:
                assert out[key].dtype == mirror[key].dtype and torch.equal(out[key], mirror[key]), key
            assert out['matching_scores'].shape[1:] == (129, 129)
            assert out['corr_scores'].shape[0] != plain(d)['corr_scores'].shape[0]
            want.append(out)
        got = net(dicts)
        for k, (g, w) in enumerate(zip(got, want)):
            for key in w:
                assert torch.equal(g[key], w[key]), (k, key)


def test_a_group_mixing_options_and_defaults_gives_each_pair_its_own_result(scene):
    """Engines of one lock-step group may differ in their options (the setting is the engine's own): every pair gets the bits
    of its own run, and the mapped host buffer of each holds its run's correspondences.  (Capacity:
    test_engine_buffers_hold_patches_with_more_than_2k_correspondences.)"""
    from rdmnet_amd import config, engine
    cfg0 = config.make_cfg()
    cfg3 = config.make_cfg()
    cfg3.fine_matching.update(topk=3, use_dustbin=False, confidence_threshold=0.0, use_global_score=True)
    e0 = engine.Engine(cfg0, scene['state'])
    e3 = engine.Engine(cfg3, None, share_with=e0)
    e0b = engine.Engine(cfg0, None, share_with=e0)
    pairs = [(torch.from_numpy(r).cuda(), torch.from_numpy(s).cuda()) for r, s in scene['clouds']]
    big = pairs[1]

    def snapshot(e):
        rc, sc, cs = e.corr()
        return e.transform(), rc.clone(), sc.clone(), cs.clone(), [x.copy() for x in e.host_corr()]

    with torch.cuda.stream(torch.cuda.Stream()):
        e3.run(*big)
        w3 = snapshot(e3)
        res = e3.result
        assert res.n_host_correspondences == res.n_correspondences == w3[1].shape[0]
        assert np.array_equal(w3[4][0], w3[1].cpu().numpy()) and np.array_equal(w3[4][1], w3[2].cpu().numpy())
        assert np.array_equal(w3[4][2], w3[3].cpu().numpy())
        e0.run(*big)
        w0 = snapshot(e0)
        e0b.run(*pairs[0])
        w0b = snapshot(e0b)
        assert w0[1].shape[0] != w3[1].shape[0]
        for _ in range(2):
            engine.Engine.run_lockstep([e0, e3, e0b], [big, big, pairs[0]])
            for e, w in ((e0, w0), (e3, w3), (e0b, w0b)):
                g = snapshot(e)
                assert np.array_equal(g[0], w[0]) and all(torch.equal(a, b) for a, b in zip(g[1:4], w[1:4]))
                assert all(np.array_equal(a, b) for a, b in zip(g[4], w[4]))


def test_engine_buffers_hold_patches_with_more_than_2k_correspondences(scene):
    """The capacity check: topk = 16 without the dustbin and threshold 0 lists up to 16 (nr + nc) correspondences per
    superpoint pair -- asserted: some pair exceeds the 2 K = 256 rows the shipped buffers give a patch -- so the per-patch
    stride, the output arrays and the mapped host buffer must all come from topk: the engine equals the operator mirror, the
    count equals the restatement's on the engine's own matching scores, and the host buffer holds every row."""
    cfg, net = make_net(scene, topk=16, use_dustbin=False, confidence_threshold=0.0)
    K = cfg.model.num_points_in_patch
    r, s = scene['clouds'][1]
    with torch.cuda.stream(torch.cuda.Stream()):
        d = scene['collate'].collate_pair(r, s, cfg)
        out, mirror = net(d), net(d, {})
        for key in ('ref_corr_points', 'src_corr_points', 'corr_scores', 'estimated_transform'):
            assert torch.equal(out[key], mirror[key]), key
        eng = net.engine()
        res = eng.result
        C = int(res.n_correspondences)
        corr = R.correspondence_matrix(R.score_matrix(out['matching_scores'].cpu(), cfg.fine_matching), out['ref_node_corr_knn_masks'].cpu(),
                                       out['src_node_corr_knn_masks'].cpu(), cfg.fine_matching)
        per_patch = corr.sum((1, 2))
        print(f'topk 16: C {C}, restatement {int(corr.sum())}, largest patch {int(per_patch.max())} (2 K = {2 * K}), '
              f'shipped host capacity {cfg.coarse_matching.num_correspondences * 2 * K}')
        assert int(per_patch.max()) > 2 * K
        assert abs(C - int(corr.sum())) <= 0.02 * C  # (exp() of the device and of torch may differ in the last bit: ties, as in the fixture)
        assert C == out['corr_scores'].shape[0] == int(res.n_host_correspondences)
        hr, hs, hc = eng.host_corr()
        assert np.array_equal(hr, out['ref_corr_points'].cpu().numpy()) and np.array_equal(hs, out['src_corr_points'].cpu().numpy())
        assert np.array_equal(hc, out['corr_scores'].cpu().numpy())
