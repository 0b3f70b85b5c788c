"""GPU: rdm_pose_graph_consistency through ops.pose_graph_consistency and `rdmnet_amd.trajectory --loop-consistency / --loop-gate`,
against the long-double inverse of tests/pose_graph_consistency_restatement.py under its criteria
(tests/test_pose_graph_consistency.py holds the host twins to the same).  Also the determinism guarantee, the statuses and the
refusals.

The placements of a pair's two nodes (tests/test_pose_graph_marginals.py: SHAPES) are covered here on the GPU too: SHAPES' systems
have no poses, so every shape's chain and chords are given poses (a drive, noisy edges) -- the separator, the runs and the couplings are
the shape's, which the test asserts through the separator's size -- and all ordered pairs of all fourteen run as one batch."""
import os

import numpy as np
import pytest
import torch

import pose_graph_cases as cases
import pose_graph_consistency_restatement as C
import pose_graph_marginals_restatement as M
import pose_graph_restatement as R
from rdmnet_amd import _lib, ops, trajectory
from test_pose_graph_marginals import SHAPES

pytestmark = pytest.mark.gpu
TERMS = 300  # as tests/test_pose_graph_consistency.py


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def call(parts, marginals=False):
    """parts: (case, weights, pairs, pair transforms or None, pair informations or None) -> one call on their concatenation, and the
    node and pair offsets."""
    noff = np.cumsum([0] + [len(p[0]['nodes']) for p in parts])
    eoff = np.cumsum([0] + [len(p[0]['edges']) for p in parts])
    poff = np.cumsum([0] + [len(p[2]) for p in parts])
    cat = lambda key: np.concatenate([p[0][key] for p in parts])
    args = (dev(cat('nodes')), cat('edges'), dev(cat('transforms')), dev(cat('informations')), dev(np.concatenate([p[1] for p in parts])))
    if marginals:
        return ops.pose_graph_marginals(*args, graph_node_offsets=noff, graph_edge_offsets=eoff)
    opt = lambda k: None if parts[0][k] is None else dev(np.concatenate([p[k] for p in parts]))
    res = ops.pose_graph_consistency(*args, pairs=np.concatenate([p[2] for p in parts]).reshape(-1, 2), pair_transforms=opt(3),
                                     pair_informations=opt(4), graph_node_offsets=noff, graph_edge_offsets=eoff, graph_pair_offsets=poff)
    return res, noff, poff


def outputs(res, nodes=slice(None), pairs=slice(None)):
    return [res.covariances[nodes], res.cross[pairs], res.residual_covariances[pairs], res.d2[pairs], res.pair_status[pairs]]


def same_bits(a, b):
    return all(torch.equal(x, y) or bool((torch.isnan(x) == torch.isnan(y)).all() and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)))
               for x, y in zip(a, b))


def part(name):
    c, w, ref, pairs, T, L = C.graph(name)
    return (c, w, pairs, T, L)


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(M.GRAPHS))
def test_pairs_match_the_long_double_inverse(name):
    c, w, ref, pairs, T, L = C.graph(name)
    res, _, _ = call([part(name)])
    assert res.status.tolist() == [0] and bool((res.pair_status == 0).all())
    for t, shape in ((res.cross, (len(pairs), 6, 6)), (res.residual_covariances, (len(pairs), 6, 6)), (res.d2, (len(pairs),))):
        assert t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_cuda
    assert torch.equal(res.covariances, call([part(name)], marginals=True).covariances)  # the same kernels in the same order
    ref.check_cross(name, pairs, res.cross.cpu().numpy())
    sub = np.arange(0, len(pairs), max(1, len(pairs) // TERMS))
    ref.check_terms(name, c['nodes'], pairs[sub], T[sub], L[sub], res.residual_covariances.cpu().numpy()[sub], res.d2.cpu().numpy()[sub])


def posed_shape(name):
    n, chords, want = SHAPES[name]
    rng = np.random.default_rng(700 + n + len(chords))
    edges = [((i, i + 1) if i % 2 else (i + 1, i)) for i in range(n - 1)] + [((s, t) if k % 2 else (t, s)) for k, (s, t) in enumerate(chords)]
    c = cases.make(cases.trajectory_truth(rng, n), edges, rng, start_angle=0.02, start_distance=0.1, noise_angle=0.01, noise_distance=0.05)
    pairs = np.array([(s, t) for s in range(n) for t in range(n) if s != t], np.int64)
    return c, np.ones(len(edges)), pairs, None, None


def test_every_placement_of_the_two_nodes_as_one_batch():
    parts = [posed_shape(name) for name in SHAPES]
    res, noff, poff = call(parts)  # pair_transforms None: the current relative poses
    assert res.status.tolist() == [0] * len(parts)
    assert res.separator.tolist() == [len(SHAPES[name][2]) for name in SHAPES]
    cross = res.cross.cpu().numpy()
    for g, name in enumerate(SHAPES):
        c = parts[g][0]
        H = M.information(c['nodes'], c['edges'], c['transforms'], c['informations'])
        C.Reference(H[6:, 6:]).check_cross(name, parts[g][2], cross[poff[g]:poff[g + 1]])
    assert float(res.d2.max()) <= 1e-20 and bool((res.pair_status == 0).all())


def test_no_pair_transforms_are_the_current_relative_poses():
    c, w, ref, pairs, T, L = C.graph('noisy')
    pairs = pairs[:60]  # (its ten loop edges and fifty of the seeded pairs)
    none, _, _ = call([(c, w, pairs, None, None)])
    assert float(none.d2.max()) <= 1e-20 and float(none.d2.min()) >= 0.0
    now = np.stack([C.current_transform(c['nodes'][s], c['nodes'][t]) for s, t in pairs])
    explicit, _, _ = call([(c, w, pairs, now, None)])
    assert float(explicit.d2.max()) <= 1e-20
    assert torch.equal(none.cross, explicit.cross) and torch.equal(none.covariances, explicit.covariances)
    ref.check_terms('noisy, current poses (None)', c['nodes'], pairs, now, None, none.residual_covariances.cpu().numpy())
    ref.check_terms('noisy, current poses (explicit)', c['nodes'], pairs, now, None, explicit.residual_covariances.cpu().numpy())


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------

def test_a_pair_s_rows_are_the_same_bits_alone_in_any_batch_with_other_pairs_and_twice():
    noisy, ring40, pair = part('noisy'), part('ring40'), part('pair')
    alone, _, _ = call([noisy])
    again, _, _ = call([noisy])
    assert same_bits(outputs(alone), outputs(again))
    first, na, pa = call([noisy, ring40, pair])
    last, nb, pb = call([ring40, pair, noisy])
    assert same_bits(outputs(first, slice(na[0], na[1]), slice(pa[0], pa[1])), outputs(alone))
    assert same_bits(outputs(last, slice(nb[2], nb[3]), slice(pb[2], pb[3])), outputs(alone))
    assert same_bits(outputs(first, slice(na[1], na[2]), slice(pa[1], pa[2])), outputs(last, slice(nb[0], nb[1]), slice(pb[0], pb[1])))
    # fewer pairs, another order: a pair's rows do not change
    c, w, pairs, T, L = noisy
    order = np.random.default_rng(4).permutation(len(pairs))[:40]
    few, _, _ = call([(c, w, pairs[order], T[order], L[order])])
    pick = torch.from_numpy(order).cuda()
    assert same_bits(outputs(few), outputs(alone, slice(None), pick))
    one, _, _ = call([(c, w, pairs[5:6], T[5:6], L[5:6])])
    assert same_bits(outputs(one), outputs(alone, slice(None), slice(5, 6)))


# ---- 3. statuses and refusals -------------------------------------------------------------------------------------------------------------

def test_a_zero_weight_that_cuts_a_node_off_is_status_4_for_its_graph_only():
    pair, tree, ring3 = part('pair'), part('tree'), part('ring3')
    cut = tree[1].copy()
    cut[-1] = 0.0  # the chain's last edge: node 49 is reached by nothing else
    few = slice(0, 60)
    res, noff, poff = call([pair, (tree[0], cut, tree[2][few], tree[3][few], tree[4][few]), ring3])
    assert res.status.tolist() == [0, 4, 0]
    mid = slice(poff[1], poff[2])
    assert torch.isnan(res.cross[mid]).all() and torch.isnan(res.residual_covariances[mid]).all() and torch.isnan(res.d2[mid]).all()
    assert torch.isnan(res.covariances[noff[1] + 1:noff[2]]).all()
    assert same_bits(outputs(res, slice(noff[0], noff[1]), slice(poff[0], poff[1])), outputs(call([pair])[0]))
    assert same_bits(outputs(res, slice(noff[2], noff[3]), slice(poff[2], poff[3])), outputs(call([ring3])[0]))


def test_an_indefinite_pair_information_is_pair_status_1():
    c, w, pairs, T, L = part('ring3')
    bad = L.copy()
    bad[2] = -bad[2]
    res, _, _ = call([(c, w, pairs, T, bad)])
    good, _, _ = call([(c, w, pairs, T, L)])
    assert res.pair_status.tolist() == [0, 0, 1, 0, 0, 0] and bool(torch.isnan(res.d2[2])) and bool(torch.isfinite(res.d2[[0, 1, 3, 4, 5]]).all())
    assert torch.equal(res.cross, good.cross) and torch.equal(res.residual_covariances, good.residual_covariances)


def test_refusals_leave_the_outputs_untouched():
    c, w, pairs, T, L = part('ring3')
    broken = T.copy()
    broken[4, 1, 3] = np.inf
    with pytest.raises(RuntimeError, match='pair 4: .*not finite'):
        call([(c, w, pairs, broken, L)])
    skewed = L.copy()
    skewed[3, 0, 5] += 1e-3
    with pytest.raises(RuntimeError, match='pair 3: .*not symmetric'):
        call([(c, w, pairs, T, skewed)])
    turned = T.copy()
    for k in (1, 5):
        turned[k, :3, :3] = turned[k, :3, :3] @ R.so3_exp(np.array([0.0, 0.0, np.pi]))
    with pytest.raises(RuntimeError, match='pair 1: .*beyond the supported angle'):
        call([(c, w, pairs, turned, L)])
    nodes = c['nodes'].copy()
    nodes[1, 0, 0] = np.nan
    with pytest.raises(RuntimeError, match='graph 0: .*not finite'):  # what the marginals call refuses comes first
        call([(dict(c, nodes=nodes), w, pairs, turned, L)])
    # the library's call itself, with every output filled beforehand
    lib = _lib.lib()
    n, p = len(c['nodes']), len(pairs)
    X, Te, Le, PT, PL = dev(c['nodes']), dev(c['transforms']), dev(c['informations']), dev(turned), dev(L)
    noff, eoff, poff = (np.array([0, k], np.int64) for k in (n, len(c['edges']), p))
    ed, pr = np.ascontiguousarray(c['edges']), np.ascontiguousarray(pairs)
    size = lib.rdm_pose_graph_consistency_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data, poff.ctypes.data, pr.ctypes.data)
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device='cuda')
    outs = [torch.full((k,), -7.0, dtype=torch.float64, device='cuda') for k in (36 * n, 36 * p, 36 * p, p)]
    status = torch.full((p,), 9, dtype=torch.uint8, device='cuda')
    report = np.full((1, 2), -7.0)

    def run(ws_bytes, pt):
        rc = lib.rdm_pose_graph_consistency(1, noff.ctypes.data, eoff.ctypes.data, X.data_ptr(), ed.ctypes.data, Te.data_ptr(), Le.data_ptr(), 0,
                                            poff.ctypes.data, pr.ctypes.data, pt.data_ptr(), PL.data_ptr(), outs[0].data_ptr(),
                                            outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), status.data_ptr(),
                                            report.ctypes.data, ws.data_ptr(), ws_bytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert run(size, PT) == -1 and 'pair 1' in lib.rdm_last_error().decode()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((status == 9).all()) and np.all(report == -7.0)
    assert run(size - 1, PT) != 0 and 'workspace too small' in lib.rdm_last_error().decode()  # the size is exact
    assert run(size, dev(T)) == 0 and np.all(report == [[0.0, 0.0]]) and all(bool(torch.isfinite(o).all()) for o in outs)
    assert bool((status == 0).all())


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------------

LOOPS = [(6, 1), (9, 3), (10, 2), (12, 5), (13, 0)]
GROSS = (10, 2)


def write_pairs(root, seq, seed, n, skip=None):
    """An odometry chain of n frames and LOOPS (src node, ref node), the pair GROSS off by 0.5 rad and 5 m; `skip`: a loop left out."""
    rng = np.random.default_rng(seed)
    truth = cases.trajectory_truth(rng, n)
    frames = [10 * i for i in range(n)]
    for s, t in [(i, i + 1) for i in range(n - 1)] + LOOPS:
        gt = cases.inverse(truth[t]) @ truth[s]
        est = R.retract(gt, cases.perturbation(rng, 0.01, 0.05))
        info = cases.random_information(rng)
        if (s, t) == GROSS:
            w = np.array([0.3, -0.3, 0.26])
            est = R.retract(est, np.concatenate([w * 0.5 / np.linalg.norm(w), [3.0, -4.0, 0.0]]))
        if (s, t) != skip:
            np.savez(str(root / f'{seq}_{frames[s]}_{frames[t]}.npz'), estimated_transform=est, transform=gt, information=info)


def run_cli(root, out, *flags):
    lines = []
    trajectory.run(trajectory.make_parser().parse_args(['--features-root', str(root), '--out', str(out), *flags]), emit=lines.append)
    return lines, {name: open(os.path.join(str(out), name), 'rb').read() for name in sorted(os.listdir(str(out)))}


def test_cli_reports_the_loop_consistency_and_gates_the_gross_edge(tmp_path):
    root, clean = tmp_path / 'pairs', tmp_path / 'clean'
    root.mkdir()
    clean.mkdir()
    write_pairs(root, 9, 31, 14)
    write_pairs(clean, 9, 31, 14, skip=GROSS)
    gross_name = f'9_{10 * GROSS[0]}_{10 * GROSS[1]}.npz'
    # without --optimize: the line and the file, beside the unchanged lines
    plain, _ = run_cli(root, tmp_path / 'plain')
    lines, files = run_cli(root, tmp_path / 'consistency', '--loop-consistency')
    print('\n'.join(lines))
    at = [k for k, l in enumerate(lines) if l.startswith('seq 9 loop consistency: ')]
    assert len(at) == 1 and [l for k, l in enumerate(lines) if k != at[0]] == plain
    rows = [r.split() for r in files['9_loop_consistency.txt'].decode().splitlines()]
    assert len(rows) == len(LOOPS)  # one row per loop edge: file, s, t, d2
    d2 = {r[0]: float(r[3]) for r in rows}
    assert sorted((int(r[1]), int(r[2])) for r in rows) == sorted(LOOPS)
    assert max(d2, key=d2.get) == gross_name
    rest = max(v for k, v in d2.items() if k != gross_name)
    words = lines[at[0]].replace(',', '').split()
    assert words[4:7] == [str(len(LOOPS)), 'loop', 'edges'] and words[7:9] == ['d2', 'median'] and words[10] == 'max'
    assert abs(float(words[9]) - np.median(list(d2.values()))) <= 1e-5 * float(words[9])
    assert abs(float(words[11]) - d2[gross_name]) <= 1e-5 * d2[gross_name] and words[12] == f'({gross_name})'
    # with a gate between the gross edge and the rest it is left out: the optimised trajectory is that of the tree without its file
    gate = float(np.sqrt(rest * d2[gross_name]))
    assert rest < gate < d2[gross_name]
    optimize = ('--optimize', '--line-process-weight', '5')
    gated, gated_files = run_cli(root, tmp_path / 'gated', *optimize, '--loop-gate', repr(gate))
    print('\n'.join(gated))
    line = [l for l in gated if l.startswith('seq 9 loop consistency: ')]
    assert len(line) == 1 and line[0].endswith(f', 1 above the gate {gate:g}')
    without, without_files = run_cli(clean, tmp_path / 'without', *optimize)
    assert gated_files['9_optimized.txt'] == without_files['9_optimized.txt']
    assert [l for l in gated if not l.startswith('seq 9 loop consistency: ')] == without  # the lines describe the graph that was optimised
    ungated, ungated_files = run_cli(root, tmp_path / 'ungated', *optimize)
    assert ungated_files['9_optimized.txt'] != gated_files['9_optimized.txt']
    assert f'{13 + len(LOOPS)} edges' in ' '.join(ungated) and f'{13 + len(LOOPS) - 1} edges' in ' '.join(gated)
