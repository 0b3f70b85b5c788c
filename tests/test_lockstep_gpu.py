"""GPU: the grouped launch of the lock-step groups (rdmnet_amd/csrc/lockstep.h) on its own, and engine groups at the sizes and
inputs the other files do not run.

Part 1 -- rdm_lockstep_selftest_gpu: the contexts of a real lock-step group launch a probe body through rdm::launch (launch_sig ->
lockstep_submit -> fire_records -> grouped_kernel, or entry_kernel for a record that found no partner) with scripted grids and
dynamic-LDS sizes.  Every workgroup of every scripted launch owns one slot of 10 int32: threads seen, visits, {tag, blockIdx,
gridDim, LDS round trip ok}.  The expectation is a plain numpy enumeration of the script; every comparison is array_equal.  THE
FIRST TWO CASES MUST STAY FIRST: they are the first launches this process makes of the probe's instantiations, with dynamic LDS
above the default limit (the limit is raised per instantiation at its first large request).

Part 2 -- groups of eight, seven and six pairs, of tiny / single-point / one-voxel-per-point clouds among ordinary ones, of a pair
that takes the deferred large-buffer search pass: every pair must give the bits of the same pair run ALONE (Engine.run / collate /
forward on another engine with the same weights -- the path tests/test_engine_gpu.py pins against the oracle and
tests/test_reference_goldens_gpu.py against the reference).  The scheduler alone (no GPU): tests/test_lockstep.py."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import small_clouds
import tie_aware

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- part 1: the grouped launch itself
WORDS = 10                      # int32 per slot (rdm_lockstep_selftest_gpu)
GUARD = 64                      # guard words before and after the slots
SENTINEL = 0x5A5A5A5A
KMAX = 160 * 1024 - 4096        # = rdm::kMaxDynamicLds
BIG = 48 * 1024                 # above rdm::kDynamicLdsDefault (32 KB): the launch has to raise the instantiation's limit
WAIT = (-1, 0, 0, 0)
GRIDS = [(1, 1, 1), (5, 1, 1), (65, 1, 1), (3, 4, 1), (1, 7, 1), (2, 3, 5), (1, 1, 9)]
LDS = [0, 1024, BIG, KMAX]


def rotating(n_ctx):
    """n_ctx scripts of 3 .. 7 steps: grids and LDS sizes rotate through GRIDS / LDS so that every grouped launch mixes them,
    odd contexts wait after their second launch, every third context has a zero-dimension step between two launches."""
    scripts = []
    for k in range(n_ctx):
        s = [GRIDS[(3 * k + 2 * i + 1) % 7] + (LDS[(k + i) % 4],) for i in range(2 + k % 4)]
        if k % 2 == 1:
            s.insert(2, WAIT)
        if k % 3 == 0:
            s.insert(1, (0, 7, 1, 0) if k % 2 == 0 else (4, 0, 1, 0))
        scripts.append(s)
    return scripts


CASES = {
    # (threads, scripts).  The first grouped launch of the 64-thread probe asks for all the LDS there is (its small-LDS record
    # first), the first launch of its own (context 0 alone, after context 1 has ended) for 48 KB ...
    'first_launches_64': (64, [[(3, 4, 1, 1024), (2, 3, 5, BIG)], [(5, 1, 1, KMAX)]]),
    # ... and the 256-thread probe the other way round
    'first_launches_256': (256, [[(1, 7, 1, BIG), (65, 1, 1, KMAX)], [(1, 1, 9, 0)]]),
    # a group of one: every launch takes the n == 1 branch of fire_records
    'one_context': (64, [[(2, 3, 5, 0), (0, 7, 1, 0), (3, 4, 1, 1024), WAIT, (1, 1, 9, KMAX), (4, 0, 1, 0), (65, 1, 1, BIG)]]),
    # a zero-dimension step is skipped without yielding: context 0's third step goes out alone, after the grouped first
    'skipped_step_then_alone': (256, [[(5, 1, 1, 0), (0, 7, 1, 0), (3, 4, 1, 1024)], [(1, 7, 1, 0)]]),
    # eight records: gy, gz > 1 at p = 0, in the middle and at p = 7; lengths 1 .. 6; waits in the middle; zero-dimension steps
    'eight_contexts': (256, [
        [(2, 3, 5, 1024), (0, 7, 1, 0), (3, 4, 1, 0), WAIT, (1, 1, 9, BIG)],
        [(5, 1, 1, 0), (1, 7, 1, 1024), WAIT, (2, 3, 5, 0)],
        [(1, 1, 1, KMAX), (65, 1, 1, 0)],
        [(3, 4, 1, BIG), (4, 0, 1, 0), (1, 1, 1, 0), WAIT, (3, 4, 1, 1024), (5, 1, 1, 0)],
        [(1, 7, 1, 0), (2, 3, 5, BIG), WAIT, (1, 1, 1, 0)],
        [(65, 1, 1, 1024), (1, 1, 9, 0), WAIT, (1, 7, 1, KMAX)],
        [(1, 1, 1, 0)],
        [(1, 1, 9, BIG), (3, 4, 1, 1024), WAIT, (2, 3, 5, 1024), WAIT, (65, 1, 1, 0)]]),
    'eight_contexts_64': (64, rotating(8)),
    'two_contexts': (64, rotating(2)),
    'five_contexts': (256, rotating(5)),
    'six_contexts': (64, rotating(6)),
    'seven_contexts': (256, rotating(7)),
}


def enumerate_slots(scripts, threads):
    """What the probe must leave behind: one row per workgroup, in the order (context, step, linear id of the step's own grid)."""
    ln = max(len(s) for s in scripts)
    rows = []
    for k, script in enumerate(scripts):
        for s, (gx, gy, gz, _) in enumerate(script):
            if gx < 0:
                continue
            for bz in range(gz):
                for by in range(gy):
                    for bx in range(gx):
                        rows.append([threads, 1, k * ln + s, bx, by, bz, gx, gy, gz, 1])
    return np.array(rows, dtype=np.int32).reshape(-1, WORDS)


def schedule(scripts):
    """The scheduler's rule (lockstep.cpp) on the script: in one pass every context that can run runs up to its next launch (a
    zero grid is no launch), wait or end; the launches recorded in a pass go out as ONE launch (one kernel per case); with
    nothing to issue the contexts that wait are released by one wait of the group.  -> (launches, records, waits)"""
    n = len(scripts)
    pos, state = [0] * n, ['ready'] * n
    launches = records = waits = 0
    while True:
        ran = False
        for k in range(n):
            if state[k] != 'ready':
                continue
            ran = True
            state[k] = 'done'
            while pos[k] < len(scripts[k]):
                gx, gy, gz, _ = scripts[k][pos[k]]
                pos[k] += 1
                if gx < 0 or gx * gy * gz > 0:
                    state[k] = 'sync' if gx < 0 else 'launch'
                    break
        for want in ('launch', 'sync'):
            m = sum(s == want for s in state)
            if m:
                launches, records, waits = launches + (want == 'launch'), records + m * (want == 'launch'), waits + (want == 'sync')
                state = ['ready' if s == want else s for s in state]
                break
        else:
            if not ran:
                return launches, records, waits


def test_the_schedule_helper_follows_the_scheduler_rule():
    # (the CPU self-test's cases, tests/test_lockstep.py, restated with one kernel)
    L, W = (1, 1, 1, 0), WAIT
    assert schedule([[L, L, L, W, L]] * 4) == (4, 16, 1)
    assert schedule([[L, W, L, W], [L]]) == (2, 3, 2)
    assert schedule([[W, L], [L, L, W, L]]) == (3, 4, 1)
    assert schedule([[L, (0, 7, 1, 0), L], [L]]) == (2, 3, 0)


@pytest.mark.parametrize('case', list(CASES))
def test_grouped_launch_runs_every_workgroup_of_every_record_once_with_its_own_arguments(case):
    from rdmnet_amd import _lib, engine
    threads, scripts = CASES[case]
    n, ln = len(scripts), max(len(s) for s in scripts)
    arr = np.zeros((n, ln, 4), dtype=np.int32)  # (a zero grid = nothing: the shorter scripts end early)
    for k, s in enumerate(scripts):
        arr[k, :len(s)] = s
    want = enumerate_slots(scripts, threads)
    slots = want.shape[0]
    buf = torch.zeros(2 * GUARD + slots * WORDS, dtype=torch.int32, device='cuda')
    buf[:GUARD] = SENTINEL
    buf[GUARD + slots * WORDS:] = SENTINEL
    torch.cuda.synchronize()
    engine.Engine.lockstep_stats(reset=True)
    got_slots = _lib.lib().rdm_lockstep_selftest_gpu(n, arr.ctypes.data, ln, threads, buf.data_ptr() + 4 * GUARD, slots, _lib.stream_ptr())
    if got_slots < 0:
        _lib.check(got_slots, 'rdm_lockstep_selftest_gpu')
    stats = engine.Engine.lockstep_stats()
    assert got_slots == slots
    got = buf.cpu().numpy()
    assert np.array_equal(got[:GUARD], np.full(GUARD, SENTINEL, np.int32)), 'written before the slots'
    assert np.array_equal(got[GUARD + slots * WORDS:], np.full(GUARD, SENTINEL, np.int32)), 'written behind the slots'
    got = got[GUARD:GUARD + slots * WORDS].reshape(slots, WORDS)
    assert np.array_equal(got[:, 1], want[:, 1]), f'visits != 1 at slots {np.nonzero(got[:, 1] != 1)[0][:16].tolist()}'
    assert np.array_equal(got[:, 0], want[:, 0]), f'threads != {threads} at slots {np.nonzero(got[:, 0] != threads)[0][:16].tolist()}'
    bad = np.nonzero((got[:, 2:] != want[:, 2:]).any(1))[0]
    assert np.array_equal(got[:, 2:], want[:, 2:]), (f'records {{tag, bx, by, bz, gx, gy, gz, lds_ok}} differ at slots {bad[:8].tolist()}: '
                                                    f'got {got[bad[:8], 2:].tolist()}, want {want[bad[:8], 2:].tolist()}')
    launches, records, waits = schedule(scripts)
    assert (stats['launches'], stats['records'], stats['waits'], stats['runs']) == (launches, records, waits, 1)


# ---------------------------------------------------------------------------------------------- part 2: engine groups
# every stage tensor an engine that keeps them knows: the tap(r, "...") sites of rdmnet_amd/csrc/engine.hip + Engine._COLLATE_NAMES
ENCODER_BLOCKS = ['1_1', '1_2', '2_1', '2_2', '2_3', '3_1', '3_2', '3_3', '4_1', '4_2', '4_3', '5_1', '5_2', '5_3']
STAGE_NAMES = ([f'points{i}' for i in range(5)] + [f'lengths{i}' for i in range(5)] + [f'neighbors{i}' for i in range(5)] +
               [f'subsampling{i}' for i in range(4)] + [f'upsampling{i}' for i in range(4)] + ['search_flags'] +
               [f'encoder.encoder{b}' for b in ENCODER_BLOCKS] +
               ['feats_c_enc', 't1', 'n2p_scores', 'decoder', 'p2p_scores', 'vote_xyz', 'vote_feats', 'nms_mask', 'nodes', 'node_scores',
                't2', 'feats_c', 'ref_node_masks', 'src_node_masks', 'ref_knn', 'src_knn', 'ref_knn_masks', 'src_knn_masks',
                'ref_node_corr_indices', 'src_node_corr_indices', 'node_corr_scores', 'patch_scores', 'matching_scores',
                'ref_node_corr_knn_points', 'src_node_corr_knn_points', 'ref_node_corr_knn_masks', 'src_node_corr_knn_masks',
                'ref_corr_points', 'src_corr_points', 'corr_scores', 'estimated_transform'])
MIXED = ['S0', 'D1', 'S1', 'D5', 'D4000', 'D50', 'S2', 'D500']  # the eight-pair group of the issue


def snapshot(e, res):
    return (e.transform().copy(), [c.clone() for c in e.corr()], int(res.n_correspondences), int(res.n_ref_nodes), int(res.n_src_nodes),
            int(res.n_node_correspondences), [int(x) for x in res.level_sizes])


def same(a, b):
    return np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and a[2:] == b[2:]


def same_result(a, b):  # pose, correspondences and counters only (no level sizes)
    return np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and a[2:6] == b[2:6]


@pytest.fixture(scope='module')
def grp(golden_dir):
    """Small inputs only; the lone-run references are computed once (on engines of their own that share the weights) and
    shared by the tests, which leave them unchanged."""
    from rdmnet_amd import config, engine, weights
    cfg = config.make_cfg()
    state = weights.synthetic_state_dict(cfg, seed=0)
    sc = np.load(os.path.join(golden_dir, 'scans.npz'))

    def crop(p, r):
        return p[np.linalg.norm(p[:, :2], axis=1) < r]
    gold = {'S0': np.load(os.path.join(golden_dir, 'forward_small.npz')), 'S1': np.load(os.path.join(golden_dir, 'forward_crop9.npz'))}
    clouds = {'S0': (gold['S0']['ref_points_in'], gold['S0']['src_points_in']), 'S1': (gold['S1']['ref_points_in'], gold['S1']['src_points_in']),
              'S2': (crop(sc['s000007'], 8.0), crop(sc['s000000'], 6.0)), 'X': small_clouds.overflow_box_pair()}
    for n, scale in small_clouds.DEGENERATE:
        clouds[f'D{n}'] = small_clouds.degenerate_pair(n, scale)
    assert all(len(a) + len(b) <= 12000 for a, b in clouds.values())
    pairs = {k: (torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()) for k, (a, b) in clouds.items()}
    lone = engine.Engine(cfg, state)  # (plain: the production form)
    want = {k: snapshot(lone, lone.run(*p)) for k, p in pairs.items()}
    engines = [engine.Engine(cfg, None, share_with=lone) for _ in range(9)]
    return dict(cfg=cfg, state=state, gold=gold, pairs=pairs, lone=lone, want=want, engines=engines, engine=engine)


def run_group(grp, engines, keys, **kw):
    res = grp['engine'].Engine.run_lockstep(engines, [grp['pairs'][k] for k in keys], **kw)
    return [snapshot(e, r) for e, r in zip(engines, res)]


def test_groups_of_eight_seven_and_six_mixed_pairs_give_every_pair_the_bits_of_its_own_run(grp):
    """Ordinary pairs and 1-point, 5-point, 50-point, 500-point and one-voxel-per-point pairs in one group: the tiny ones skip
    launches, end early, have zero-row tensors and wait at other places than the rest."""
    engines, want = grp['engines'], grp['want']
    with torch.cuda.stream(torch.cuda.Stream()):
        for collated in (True, False):
            for keys in (MIXED, MIXED[1:], MIXED[2:], MIXED[::-1]):
                got = run_group(grp, engines, keys, collate_batched=collated)
                for k, key in enumerate(keys):
                    assert same(got[k], want[key]), (collated, len(keys), k, key)
        # an engine of the groups runs alone again afterwards
        assert same(snapshot(engines[3], engines[3].run(*grp['pairs']['S2'])), want['S2'])
        assert same(snapshot(engines[0], engines[0].run(*grp['pairs']['D1'])), want['D1'])


def test_group_of_eight_holds_every_stage_tensor_of_every_pair(grp):
    """Engines that keep their stage tensors, in the mixed group of eight: EVERY stage tensor of every engine equals that of the
    pair's own run, zero-row tensors included -- a failure names (pair, stage)."""
    engine = grp['engine']
    lone = engine.Engine(grp['cfg'], None, share_with=grp['lone'])
    lone.keep_taps(True)
    assert set(engine.Engine._COLLATE_NAMES) <= set(STAGE_NAMES) and len(set(STAGE_NAMES)) == len(STAGE_NAMES)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rdmnet_amd', 'csrc', 'engine.hip')).read()
    literal = set(re.findall(r'\btap\(\w+, "([A-Za-z0-9_.]+)"', src))
    assert len(literal) >= 30 and literal <= set(STAGE_NAMES), sorted(literal - set(STAGE_NAMES))  # (a new tap site belongs in the list)
    want = {}
    for key in MIXED:
        lone.run(*grp['pairs'][key])
        want[key] = {n: t.clone() for n, t in lone.tensors(STAGE_NAMES).items()}  # (rdm_engine_describe: an unknown name raises)
    engines = [engine.Engine(grp['cfg'], None, share_with=grp['lone']) for _ in range(8)]
    for e in engines:
        e.keep_taps(True)
    with torch.cuda.stream(torch.cuda.Stream()):
        got = run_group(grp, engines, MIXED)
        differ = []  # (pair, stage) of every tensor that is not the lone run's
        for k, key in enumerate(MIXED):
            mine = engines[k].tensors(STAGE_NAMES)
            for n in STAGE_NAMES:
                if mine[n].dtype != want[key][n].dtype or mine[n].shape != want[key][n].shape or not torch.equal(mine[n], want[key][n]):
                    differ.append((key, n))
        assert not differ, differ
        for k, key in enumerate(MIXED):
            assert same(got[k], grp['want'][key]), (k, key)


def test_a_pair_that_takes_the_deferred_large_buffer_pass_in_a_group_of_pairs_that_have_none(grp):
    engines, want = grp['engines'], grp['want']
    with torch.cuda.stream(torch.cuda.Stream()):
        for collated in (True, False):
            keys = ['X', 'S0', 'D1']
            got = run_group(grp, engines, keys, collate_batched=collated)
            for k, key in enumerate(keys):
                assert same(got[k], want[key]), (collated, k, key)


def test_collate_and_forward_entry_points_at_eight(grp):
    """collate_lockstep / forward_lockstep (the drop-in API's two halves) on the mixed group of eight against collate / forward on
    every pair alone.  rdm_engine_forward's check of a data_dict (check_data_dict, engine.hip) wants at least two points and one
    per cloud at every level: the single-point pair's dict (2 points, 1 + 1, at all five levels) passes it, so all eight run."""
    engine = grp['engine']
    lone = engine.Engine(grp['cfg'], None, share_with=grp['lone'])
    engines = [engine.Engine(grp['cfg'], None, share_with=grp['lone']) for _ in range(8)]
    pairs = [grp['pairs'][k] for k in MIXED]
    with torch.cuda.stream(torch.cuda.Stream()):
        want_d = [lone.collate(r, s) for r, s in pairs]
        got_d = engine.Engine.collate_lockstep(engines, pairs)
        assert len(got_d) == 8
        for key, g, w in zip(MIXED, got_d, want_d):
            assert g['_level_ref_sizes'] == w['_level_ref_sizes'], key
            assert torch.equal(g['features'], w['features']) and torch.equal(g['_flags'], w['_flags']), key
            for name in ('points', 'lengths', 'neighbors', 'subsampling', 'upsampling'):
                assert len(g[name]) == len(w[name]), (key, name)
                for i, (a, c) in enumerate(zip(g[name], w[name])):
                    assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a, c), (key, name, i)
        d1 = got_d[MIXED.index('D1')]
        assert [int(p.shape[0]) for p in d1['points']] == [2] * 5 and d1['_level_ref_sizes'] == [1] * 5
        assert all(t.shape[1] >= 1 for name in ('neighbors', 'subsampling', 'upsampling') for t in d1[name])
        want_f = [snapshot(lone, lone.forward(d)) for d in want_d]
        res = engine.Engine.forward_lockstep(engines, got_d)
        for k, key in enumerate(MIXED):
            assert same(snapshot(engines[k], res[k]), want_f[k]), (k, key)
            assert same(want_f[k], grp['want'][key]), (k, key)  # (collate + forward = run)


@pytest.mark.parametrize('variant', ['bf16_attention', 'vote_off'])
def test_configuration_variants_at_eight(grp, variant):
    """bf16 attention (another attention instantiation in the grouped launches) and the vote-off mode (another launch sequence)
    on the mixed group of eight: pose, correspondences and counters of every pair equal its own run."""
    engine = grp['engine']
    cfg = copy.deepcopy(grp['cfg'])
    if variant == 'bf16_attention':
        cfg.thdroformer.attention_bf16 = True
    else:
        cfg.Vote.inference_use_vote = False
    lone = engine.Engine(cfg, grp['state'])
    engines = [engine.Engine(cfg, None, share_with=lone) for _ in range(8)]
    want = [snapshot(lone, lone.run(*grp['pairs'][k])) for k in MIXED]
    assert not all(same_result(w, grp['want'][k]) for w, k in zip(want, MIXED))  # (the variant really computes something else)
    with torch.cuda.stream(torch.cuda.Stream()):
        got = run_group(grp, engines, MIXED)
        for k, key in enumerate(MIXED):
            assert same_result(got[k], want[k]), (k, key)


def test_identical_pairs_are_grouped_completely(grp):
    """Eight times the same pair, each collated inside the group: identical contexts record the same kernel in every pass, so
    every launch the scheduler issues carries eight records.  The mixed group must at least group something."""
    engine, engines = grp['engine'], grp['engines']
    with torch.cuda.stream(torch.cuda.Stream()):
        engine.Engine.lockstep_stats(reset=True)
        got = run_group(grp, engines, ['S1'] * 8, collate_batched=False)
        stats = engine.Engine.lockstep_stats(reset=True)
        assert all(same(g, grp['want']['S1']) for g in got)
        assert stats['runs'] == 1 and stats['launches'] > 100, stats
        assert stats['records'] == 8 * stats['launches'], stats
        run_group(grp, engines, MIXED)
        stats = engine.Engine.lockstep_stats(reset=True)
        assert stats['records'] > stats['launches'] > 0, stats


def test_nine_pairs_are_refused_and_the_engines_still_run_eight(grp):
    engines, want = grp['engines'], grp['want']
    assert len(engines) == 9
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(RuntimeError, match=r'1 \.\. 8 pairs'):
            run_group(grp, engines, MIXED + ['S0'])
        got = run_group(grp, engines, MIXED)
        for k, key in enumerate(MIXED):
            assert same(got[k], want[key]), (k, key)


def test_poses_of_the_golden_pairs_inside_the_group_match_the_reference(grp):
    """The anchor outside this library: `small` and `crop9` inside the mixed group of eight against the poses the REFERENCE
    returned for them (tests/golden/forward_*.npz) -- metric and bound of tests/test_reference_goldens_gpu.py for these two
    cases: the pose must match one of the reference's poses from the hypotheses within one inlier of its best
    (`lgr/alt_transforms`) within RRE <= 1e-3 deg and RTE <= 1e-5 m."""
    engines = grp['engines']
    with torch.cuda.stream(torch.cuda.Stream()):
        run_group(grp, engines, MIXED)
    for key in ('S0', 'S1'):
        g = grp['gold'][key]
        assert int(g['weight_seed']) == 0
        T = engines[MIXED.index(key)].transform()
        errs = [tie_aware.rre_rte(T, A) for A in g['lgr/alt_transforms']]
        rre, rte = errs[int(np.argmin([e[0] for e in errs]))]
        assert rre <= 1e-3 and rte <= 1e-5, (key, rre, rte)
