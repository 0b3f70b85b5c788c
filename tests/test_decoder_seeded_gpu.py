"""GPU: the decoder stage that multiplies the coarse rows once (P = coarse W[0:c1]) and seeds the skip half's product with
P[idx[m]] returns the bits of the materialised route (rdm_upsample_concat into a buffer, then the plain product /
rdm_linear_group_norm on it): an output element is one fp32 fma chain over ascending k whichever route forms it.

Every case asserts torch.equal against the materialised route AND closeness to a float64 reference at the tolerance
tests/test_ops_gpu.py uses for decoder stages (2e-5 of the output range).  Which route a call took is read off the workspace:
the region past rdm_linear_group_norm_workspace_bytes holds P (or the concatenated rows) and stays untouched otherwise."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sampling import sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from rdmnet_amd import ops
    return ops


def padded(t, device='cuda'):
    """[n, c] tensor -> device view with row stride padded to a multiple of 4 (pads zeroed)."""
    n, c = t.shape
    ld = (c + 3) // 4 * 4
    buf = torch.zeros((n, ld), dtype=torch.float32, device=device)
    buf[:, :c] = t.to(device)
    return buf[:, :c]


def last_plan():
    from rdmnet_amd import _lib
    out = (ctypes.c_int * 4)()
    _lib.check(_lib.lib().rdm_gemm_last_plan(ctypes.addressof(out)), 'rdm_gemm_last_plan')
    return list(out)


def decoder_stage(ops, coarse, idx, skip, w, n, bias, gamma=None, beta=None, groups=8):
    """rdm_decoder_stage on a zeroed workspace of its own -> (result, plan of its last product, whether the workspace region
    behind the Linear + GroupNorm scratch was written: P on the seeded route, the concatenated rows on the materialised one)."""
    from rdmnet_amd import _lib
    L = _lib.lib()
    m, c1, c2 = skip.shape[0], coarse.shape[1], skip.shape[1]
    lin = ops.feat_empty(m, n, skip.device)
    y = ops.feat_empty(m, n, skip.device) if gamma is not None else None
    ws = torch.zeros(L.rdm_decoder_stage_workspace_bytes(m, n, c1 + c2), dtype=torch.uint8, device=skip.device)
    _lib.check(L.rdm_decoder_stage(coarse.data_ptr(), coarse.shape[0], c1, coarse.stride(0), idx.data_ptr(), idx.stride(0),
                                   skip.data_ptr(), c2, skip.stride(0), m, w.data_ptr(), w.stride(0), _lib.ptr(bias), n, groups,
                                   _lib.ptr(gamma), _lib.ptr(beta), 1e-5, ops.ACT_LEAKY if gamma is not None else ops.ACT_NONE,
                                   lin.data_ptr(), lin.stride(0), _lib.ptr(y), y.stride(0) if y is not None else 0,
                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_decoder_stage')
    plan = last_plan()
    wrote = bool(ws[L.rdm_linear_group_norm_workspace_bytes(m, n) - 1024:].any().item())  # (its last 1024 bytes are slack)
    return (y if gamma is not None else lin), plan, wrote


def materialised(ops, coarse, idx, skip, w, kpad, n, bias, gamma=None, beta=None, groups=8):
    cat = ops.upsample_concat(coarse, idx, skip)
    if gamma is None:
        return ops.gemm(cat, w, kpad, n, bias=bias)
    return ops.linear_group_norm(cat, w, kpad, n, bias, gamma, beta, groups, act=ops.ACT_LEAKY)


def make_case(seed, m, n_coarse, c1, c2, n_w, idx0=None):
    """Operands of one stage: the weight has n_w columns (row stride pad4(n_w)); idx has 5 columns of which column 0 counts."""
    g = torch.Generator().manual_seed(seed)
    k = c1 + c2
    coarse, skip = torch.randn(n_coarse, c1, generator=g), torch.randn(m, c2, generator=g)
    idx = torch.randint(-3, n_coarse + 4, (m, 5), generator=g)  # (the other columns: anything)
    idx[:, 0] = idx0 if idx0 is not None else torch.randint(0, n_coarse + 1, (m,), generator=g)  # includes the shadow index
    w, bias = torch.randn(k, n_w, generator=g) / k ** 0.5, torch.randn(n_w, generator=g)
    gamma, beta = torch.rand(n_w, generator=g) + 0.5, torch.randn(n_w, generator=g)
    kpad = (k + 3) // 4 * 4
    wp = torch.zeros(kpad, n_w)
    wp[:k] = w
    i0 = idx[:, 0]
    rows = torch.cat([coarse, torch.zeros(1, c1)])[torch.where((i0 >= 0) & (i0 < n_coarse), i0, torch.full_like(i0, n_coarse))]
    a64 = torch.cat([rows, skip], 1).double()
    dev = dict(coarse=padded(coarse), idx=idx.cuda(), skip=padded(skip), w=padded(wp), bias=bias.cuda(), gamma=gamma.cuda(),
               beta=beta.cuda())
    return dict(dev=dev, a64=a64, w64=w.double(), bias64=bias.double(), gamma64=gamma.double(), beta64=beta.double(), kpad=kpad)


def want64(c, n, norm, groups=8):
    lin = c['a64'] @ c['w64'][:, :n] + c['bias64'][:n]
    if not norm:
        return lin
    return F.leaky_relu(F.group_norm(lin.t()[None], groups, c['gamma64'][:n], c['beta64'][:n], 1e-5)[0].t(), 0.1)


def run_both(ops, c, n, norm):
    d = c['dev']
    extra = (d['gamma'], d['beta']) if norm else ()
    got, plan, wrote = decoder_stage(ops, d['coarse'], d['idx'], d['skip'], d['w'], n, d['bias'], *extra)
    sep = materialised(ops, d['coarse'], d['idx'], d['skip'], d['w'], c['kpad'], n, d['bias'], *extra)
    want = want64(c, n, norm)
    err = (got.cpu().double() - want).abs().max().item()
    print(f'n={n} norm={norm}: plan {plan}, workspace tail written {wrote}, max err {err:.3e} (bound {2e-5 * want.abs().max().item():.3e}), '
          f'differing elements vs the materialised route {int((got != sep).sum().item())}')
    assert torch.equal(got, sep)
    assert err <= 2e-5 * want.abs().max().item()
    return got, plan, wrote


@pytest.mark.parametrize('norm', [True, False])
def test_ragged_tiles_and_k(ops, norm):
    """m = 130 (ragged last row tile), n = 72 (ragged column tile), c2 = 36 (no multiple of the 32-deep k-tile), 37 coarse rows;
    with GroupNorm + LeakyReLU and statistics (8 groups of 9 channels), and bias only."""
    c = make_case(1, 130, 37, 64, 36, 72)
    _, plan, wrote = run_both(ops, c, 72, norm)
    assert plan == [64, 64, 32, 1] and wrote  # (the seeded product, un-split; P was written)


@pytest.mark.parametrize('norm', [True, False])
def test_shadow_rows_and_shared_parents(ops, norm):
    """Row tile 0 is all shadow rows (index n_coarse and negative ones), tile 1 mixes shadow and real rows, the rest share five
    parents; the last tile is ragged."""
    m, n_coarse = 200, 5
    g = torch.Generator().manual_seed(7)
    i0 = torch.randint(0, n_coarse, (m,), generator=g)
    i0[:64] = torch.where(torch.arange(64) % 2 == 0, torch.tensor(n_coarse), torch.tensor(-1))
    i0[64:128:3] = n_coarse
    i0[65:128:7] = -2
    i0[70] = n_coarse + 9
    c = make_case(2, m, n_coarse, 64, 36, 72, idx0=i0)
    got, plan, wrote = run_both(ops, c, 72, norm)
    assert plan == [64, 64, 32, 1] and wrote
    if not norm:  # a shadow row's coarse half is +0: the row is the skip half's own product
        d = c['dev']
        only_skip = ops.gemm(d['skip'], d['w'][64:], 36, 72, bias=d['bias'])
        assert torch.equal(got[:64], only_skip[:64])


def test_256_of_257_columns_share_the_weight(ops):
    """n = 257 and n = 256 from one 257-column weight (the row stride stays 260): the first 256 columns are the same bits."""
    c = make_case(3, 130, 37, 64, 36, 257)
    full, plan_f, wrote_f = run_both(ops, c, 257, False)
    part, plan_p, wrote_p = run_both(ops, c, 256, False)
    assert plan_f == plan_p == [64, 64, 32, 1] and wrote_f and wrote_p
    assert full.shape[1] == 257 and part.shape[1] == 256
    assert torch.equal(full[:, :256], part)


def test_fallbacks_keep_the_old_route(ops):
    # as many coarse rows as fine rows: nothing to save, the concatenating product runs (workspace tail untouched)
    c = make_case(4, 130, 130, 64, 36, 72)
    _, plan, wrote = run_both(ops, c, 72, True)
    assert plan == [64, 64, 32, 1] and not wrote
    c = make_case(5, 130, 200, 64, 36, 72)
    _, _, wrote = run_both(ops, c, 72, False)
    assert not wrote
    # c1 = 48 is no multiple of the k-tile: the materialised route itself (the concatenated rows are in the workspace)
    c = make_case(6, 130, 37, 48, 36, 72)
    _, _, wrote = run_both(ops, c, 72, True)
    assert wrote
    # a product the planner splits over K (300 rows, k = 2112) stays the concatenated split-K product
    c = make_case(8, 300, 100, 2048, 64, 72)
    _, plan, wrote = run_both(ops, c, 72, True)
    assert plan[:2] == [64, 64] and plan[3] > 1 and not wrote
    _, plan, wrote = run_both(ops, c, 72, False)
    assert plan[3] > 1 and not wrote


@pytest.mark.parametrize('tag', ['small', 'synth0'])
def test_engine_plain_run_equals_run_with_stage_tensors(golden_dir, tag):
    """A plain run reads 256 of decoder2's 257 columns (and computes only those where the product runs un-split: the full-size
    pair; the small crop's runs split-K and keeps all), a run that keeps its stage tensors all of them: same pose, same
    correspondences; the kept `decoder` tensor has its 257 columns and matches the recorded one (2e-5, as the golden test)."""
    from rdmnet_amd import config, engine, weights
    cfg = config.make_cfg()
    g = np.load(os.path.join(golden_dir, f'forward_{tag}.npz'))
    rp, sp = torch.from_numpy(g['ref_points_in']).cuda(), torch.from_numpy(g['src_points_in']).cuda()
    eng = engine.Engine(cfg, weights.synthetic_state_dict(cfg, seed=int(g['weight_seed'])))
    eng.run(rp, sp)  # plain
    T0, corr0 = eng.transform().copy(), [x.cpu().clone() for x in eng.corr()]
    eng.keep_taps(True)
    eng.run(rp, sp)
    assert np.array_equal(eng.transform(), T0)
    for a, b in zip(eng.corr(), corr0):
        assert torch.equal(a.cpu(), b)
    dec = eng.tensor('decoder').cpu().numpy()
    assert dec.shape[1] == 257
    want = g['tap/decoder'].astype(np.float64)
    rel = np.abs(sample(dec).astype(np.float64) - want).max() / np.abs(want).max()
    print(f'decoder tap vs the recorded one: {rel:.3e}')
    assert rel <= 2e-5
    p2p = eng.tensor('p2p_scores').cpu().numpy().reshape(-1)
    assert np.allclose(p2p, 1.0 / (1.0 + np.exp(-dec[:, 256].astype(np.float64))), rtol=0, atol=1e-6)
    eng.keep_taps(False)
    eng.run(rp, sp)  # and plain again on the same engine
    assert np.array_equal(eng.transform(), T0)
