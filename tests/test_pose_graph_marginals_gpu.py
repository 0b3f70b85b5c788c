"""GPU: rdm_pose_graph_marginals through ops.pose_graph_marginals and `rdmnet_amd.trajectory --optimize --covariance`, against the
long-double inverse of tests/pose_graph_marginals_restatement.py under its accuracy criterion (the largest per-block relative error
<= max(10 x np.linalg.inv's on the same matrix, 1e-14); tests/test_pose_graph_marginals.py holds the host twin to the same).  Also
the determinism guarantee, the per-graph status, the weights and the refusals."""
import os

import numpy as np
import pytest
import torch

import pose_graph_cases as cases
import pose_graph_marginals_restatement as M
import pose_graph_restatement as R
from rdmnet_amd import _lib, ops, trajectory

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def marginals(c, weights=None, nodes=None, **kw):
    return ops.pose_graph_marginals(dev(c['nodes'] if nodes is None else nodes), c['edges'], dev(c['transforms']), dev(c['informations']),
                                    weights, **kw)


def batch(parts):
    """parts: (case, weights) -> the arguments of one call on their concatenation."""
    noff = np.cumsum([0] + [len(c['nodes']) for c, _ in parts])
    eoff = np.cumsum([0] + [len(c['edges']) for c, _ in parts])
    cat = lambda key: np.concatenate([c[key] for c, _ in parts])
    res = ops.pose_graph_marginals(dev(cat('nodes')), cat('edges'), dev(cat('transforms')), dev(cat('informations')),
                                   dev(np.concatenate([w for _, w in parts])), graph_node_offsets=noff, graph_edge_offsets=eoff)
    return res, noff


SEPARATOR = dict(pair=0, ring3=0, double=0, tree=0, ring40=3, noisy=8, gross=8, noisy100=12)


@pytest.mark.parametrize('name', list(M.GRAPHS))
def test_marginals_match_the_long_double_inverse(name):
    c, w, ref = M.graph(name)
    res = marginals(c, dev(w))
    assert res.covariances.dtype == torch.float64 and tuple(res.covariances.shape) == (len(c['nodes']), 6, 6) and res.covariances.is_cuda
    assert res.status.tolist() == [0] and res.separator.tolist() == [SEPARATOR[name]]
    ref.check(name, res.covariances.cpu().numpy())


def test_closed_form_one_edge_at_zero_residual():
    c, L = M.closed_form()
    res = marginals(c)
    M.Reference(0.5 * (L + L.T)).check('closed form', res.covariances.cpu().numpy())  # H^-1, not (2 H)^-1; rotation first


def test_a_graph_s_covariances_are_the_same_bits_alone_in_any_batch_and_twice():
    noisy, ring40, pair = (M.graph(k)[:2] for k in ('noisy', 'ring40', 'pair'))
    alone = marginals(noisy[0], dev(noisy[1])).covariances
    again = marginals(noisy[0], dev(noisy[1])).covariances
    assert torch.equal(alone, again)
    first, off_a = batch([noisy, ring40, pair])
    last, off_b = batch([ring40, pair, noisy])
    assert first.status.tolist() == [0, 0, 0] and first.separator.tolist() == [8, 3, 0] and last.separator.tolist() == [3, 0, 8]
    assert torch.equal(first.covariances[off_a[0]:off_a[1]], alone)
    assert torch.equal(last.covariances[off_b[2]:off_b[3]], alone)
    assert torch.equal(first.covariances[off_a[1]:off_a[2]], last.covariances[off_b[0]:off_b[1]])
    assert torch.equal(first.covariances[off_a[2]:off_a[3]], marginals(pair[0], dev(pair[1])).covariances)


def test_a_zero_weight_that_cuts_a_node_off_is_status_4_for_its_graph_only():
    pair, tree, ring3 = (M.graph(k)[:2] for k in ('pair', 'tree', 'ring3'))
    cut = tree[1].copy()
    cut[-1] = 0.0  # the chain's last edge: node 49 is reached by nothing else
    res, off = batch([pair, (tree[0], cut), ring3])
    assert res.status.tolist() == [0, 4, 0]
    cov = res.covariances
    assert torch.all(cov[off[1]] == 0.0) and torch.isnan(cov[off[1] + 1:off[2]]).all()
    assert torch.equal(cov[off[0]:off[1]], marginals(pair[0], dev(pair[1])).covariances)
    assert torch.equal(cov[off[2]:off[3]], marginals(ring3[0], dev(ring3[1])).covariances)
    # graphs without edges: several nodes are status 4, one node or none is status 0
    empty = ops.pose_graph_marginals(dev(np.stack([np.eye(4)] * 4)), np.zeros((0, 2), np.int64), dev(np.zeros((0, 4, 4))),
                                     dev(np.zeros((0, 6, 6))), graph_node_offsets=[0, 3, 4, 4], graph_edge_offsets=[0, 0, 0, 0])
    assert empty.status.tolist() == [4, 0, 0]
    assert torch.all(empty.covariances[0] == 0.0) and torch.isnan(empty.covariances[1:3]).all() and torch.all(empty.covariances[3] == 0.0)


def test_the_optimiser_s_weights_go_straight_in_and_none_is_all_ones():
    c = cases.noisy(gross=3)
    res = ops.pose_graph_optimize(dev(c['nodes']), c['edges'], dev(c['transforms']), dev(c['informations']), c['uncertain'],
                                  line_process_weight=1.0)
    assert res.weights.is_cuda and float(res.weights.min()) < 0.25  # the gross loop edge is weighted down
    got = ops.pose_graph_marginals(res.nodes, c['edges'], dev(c['transforms']), dev(c['informations']), res.weights)
    assert got.status.tolist() == [0]
    nodes, w = res.nodes.cpu().numpy(), res.weights.cpu().numpy()
    ref = M.Reference(M.information(nodes, c['edges'], c['transforms'], c['informations'], w)[6:, 6:])
    ref.check('gross at the optimum', got.covariances.cpu().numpy())
    ring = M.graph('ring40')[0]
    assert torch.equal(marginals(ring).covariances, marginals(ring, dev(np.ones(len(ring['edges'])))).covariances)


def test_refusals_leave_the_output_untouched():
    c = cases.consistent('ring3')
    nodes = c['nodes'].copy()
    nodes[1, 0, 0] = np.nan
    with pytest.raises(RuntimeError, match='not finite'):
        marginals(c, nodes=nodes)
    turned = c['nodes'].copy()
    turned[2, :3, :3] = turned[2, :3, :3] @ R.so3_exp(np.array([0.0, 0.0, np.pi]))
    with pytest.raises(RuntimeError, match='beyond the supported angle'):
        marginals(c, nodes=turned)
    # a negative weight past the Python layer's check: the library's own refusal
    L = _lib.lib()
    X, T, Lm, W = dev(c['nodes']), dev(c['transforms']), dev(c['informations']), dev(np.array([1.0, -1.0, 1.0]))
    out = torch.full((3, 36), -7.0, dtype=torch.float64, device='cuda')
    noff, eoff, ed = np.array([0, 3], np.int64), np.array([0, 3], np.int64), np.ascontiguousarray(c['edges'])
    size = L.rdm_pose_graph_marginals_workspace_bytes(1, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data)
    ws = torch.empty(size, dtype=torch.uint8, device='cuda')
    report = np.full((1, 2), -7.0)
    rc = L.rdm_pose_graph_marginals(1, noff.ctypes.data, eoff.ctypes.data, X.data_ptr(), ed.ctypes.data, T.data_ptr(), Lm.data_ptr(),
                                    W.data_ptr(), out.data_ptr(), report.ctypes.data, ws.data_ptr(), size, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and 'weight' in L.rdm_last_error().decode() and 'graph 0' in L.rdm_last_error().decode()
    assert torch.all(out == -7.0) and np.all(report == -7.0)
    rc = L.rdm_pose_graph_marginals(1, noff.ctypes.data, eoff.ctypes.data, X.data_ptr(), ed.ctypes.data, T.data_ptr(), Lm.data_ptr(),
                                    W.data_ptr(), out.data_ptr(), report.ctypes.data, ws.data_ptr(), size - 1, _lib.stream_ptr())
    assert rc != 0 and 'workspace too small' in L.rdm_last_error().decode()  # the size is exact


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def write_pairs(root, seq, seed, n, loop):
    rng = np.random.default_rng(seed)
    truth = cases.trajectory_truth(rng, n)
    frames = [10 * i for i in range(n)]
    pairs = [(i, i + 1) for i in range(n - 1)] + ([(n - 1, 0)] if loop else [])  # (src node, ref node)
    for s, t in pairs:
        gt = cases.inverse(truth[t]) @ truth[s]
        est = R.retract(gt, cases.perturbation(rng, 0.01, 0.05))
        np.savez(str(root / f'{seq}_{frames[s]}_{frames[t]}.npz'), estimated_transform=est, transform=gt,
                 information=cases.random_information(rng))


def run_cli(root, out, *flags):
    lines = []
    args = trajectory.make_parser().parse_args(['--features-root', str(root), '--optimize', '--line-process-weight', '5', '--out', str(out),
                                                *flags])
    trajectory.run(args, emit=lines.append)
    return lines, {name: open(os.path.join(str(out), name), 'rb').read() for name in sorted(os.listdir(str(out)))}


def test_cli_reports_and_writes_the_covariance(tmp_path):
    """Sequence 9 is an open chain of 12 frames (nearly straight: sigma grows along it), sequence 10 a ring of 12 (the loop pulls
    the last frames' sigma down)."""
    root = tmp_path / 'pairs'
    root.mkdir()
    write_pairs(root, 9, 21, 12, loop=False)
    write_pairs(root, 10, 22, 12, loop=True)
    plain, plain_files = run_cli(root, tmp_path / 'plain')
    lines, files = run_cli(root, tmp_path / 'cov', '--covariance')
    print('\n'.join(lines))
    # without the flag nothing changes: the other lines and files are the same bytes
    assert [l for l in lines if 'optimized uncertainty' not in l] == plain
    assert {k: v for k, v in files.items() if 'covariance' not in k} == plain_files
    assert sorted(set(files) - set(plain_files)) == ['10_optimized_covariance.txt', '9_optimized_covariance.txt']
    sigma = {}
    for seq in (9, 10):
        at = [k for k, l in enumerate(lines) if l.startswith(f'seq {seq} optimized uncertainty: ')]
        assert len(at) == 1 and lines[at[0] - 1].startswith(f'seq {seq} pose graph: ')
        words = lines[at[0]].replace(';', '').replace(',', '').split()
        # ... position sigma median A m max B m at frame F rotation sigma median C deg max D deg at frame F'
        assert words[4:7] == ['position', 'sigma', 'median'] and words[8:10] == ['m', 'max'] and words[11:14] == ['m', 'at', 'frame']
        assert words[15:18] == ['rotation', 'sigma', 'median'] and words[19:21] == ['deg', 'max'] and words[22:25] == ['deg', 'at', 'frame']
        cov = np.loadtxt(str(tmp_path / 'cov' / f'{seq}_optimized_covariance.txt')).reshape(-1, 6, 6)
        assert cov.shape == (12, 6, 6) and np.all(cov[0] == 0.0) and np.array_equal(cov, cov.transpose(0, 2, 1))
        pos = np.sqrt(np.trace(cov[:, 3:, 3:], axis1=1, axis2=2))
        rot = np.degrees(np.sqrt(np.trace(cov[:, :3, :3], axis1=1, axis2=2)))
        for value, want in ((words[7], np.median(pos)), (words[10], pos.max()), (words[18], np.median(rot)), (words[21], rot.max())):
            assert abs(float(value) - want) <= 1e-5 * want
        assert int(words[14]) == int(np.argmax(pos)) and int(words[25]) == int(np.argmax(rot))
        sigma[seq] = (pos, rot)
    pos, rot = sigma[9]
    assert np.all(np.diff(pos) > 0.0) and np.all(np.diff(rot) > 0.0)  # dead reckoning: every frame is known worse than the one before
    pos, rot = sigma[10]
    assert 0 < int(np.argmax(pos)) < 11 and pos[11] < 0.7 * pos.max() and rot[11] < 0.7 * rot.max()  # the loop ties the end to the start


def test_cli_covariance_needs_optimize(tmp_path):
    args = trajectory.make_parser().parse_args(['--features-root', str(tmp_path), '--covariance'])
    with pytest.raises(trajectory.TrajectoryError, match='--covariance needs --optimize'):
        trajectory.run(args)
