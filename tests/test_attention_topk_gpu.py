"""GPU: top-k attention (rdm_attention_topk / rdm_attention_self_pair_topk, cfg.thdroformer.k2) through the C-ABI
(rdmnet_amd.ops) against a float64 restatement of the reference's dynamic_attention (rdmnet/thdroformer/thdroformer.py:20-40):
scores q k^T / sqrt(32) from the same fp32 q and k, the `keep` largest kept (ties: lowest key index, as the header defines),
softmax over the kept scores, P V.

The kernel's selection is read back exactly: with one head's q and k repeated over H = ceil(nk / 32) heads and v the
identity (v[j, j] = 1), output column j of a query row is that row's probability of key j -- zero exactly where the key
is not kept (randn scores are far from exp underflow).  Rows whose k-th / (k+1)-th fp64 score gap is within the fp32
error of the scores are excluded from the set comparison (derived in `clear_rows`)."""
import numpy as np
import pytest
import torch

from oracle import forward as ofw
from test_heads_gpu import U, attention_tolerance, strided

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 331, 450, 2048, 5000]


@pytest.fixture(scope='module')
def ops():
    from rdmnet_amd import ops
    return ops


def scores64(q, k, heads):
    """[heads, nq, nk] fp64 scores of the fp32 operands."""
    qh, kh = ofw._heads(q.double(), heads), ofw._heads(k.double(), heads)
    return torch.einsum('hnd,hmd->hnm', qh, kh) / 32 ** 0.5


def select64(s, keep):
    """[..., nk] scores -> bool mask of the `keep` largest per row, ties to the lowest index."""
    nk = s.shape[-1]
    order = np.lexsort((np.broadcast_to(np.arange(nk), s.shape), -s.numpy()), axis=-1)
    mask = np.zeros(s.shape, bool)
    np.put_along_axis(mask, order[..., :keep], True, axis=-1)
    return torch.from_numpy(mask)


def topk_fp64(q, k, v, heads, keep, sel=None):
    """dynamic_attention in fp64 -> [nq, heads * 32]; `sel` overrides the selected set."""
    s = scores64(q, k, heads)
    sel = select64(s, keep) if sel is None else sel
    if keep == 0:
        return torch.zeros(q.shape[0], q.shape[1], dtype=torch.float64)
    p = torch.where(sel, s - s.amax(-1, keepdim=True), torch.tensor(-np.inf, dtype=torch.float64)).exp()
    p = p / p.sum(-1, keepdim=True)
    o = p @ ofw._heads(v.double(), heads)
    return o.transpose(0, 1).reshape(q.shape[0], -1)


def clear_rows(q, k, heads, keep):
    """[nq] bool: rows whose selection every fp32 evaluation of the scores agrees on.  A kernel score is a 32-term fp32 dot
    product divided by sqrt(32): off from the fp64 value by at most (32 + 2) u A_row, A_row = max_j sum_i |q_i k_ji| /
    sqrt(32); the k-th and (k+1)-th scores can swap only when their fp64 gap is at most twice that."""
    nk = k.shape[0]
    if keep == 0 or keep >= nk:
        return torch.ones(q.shape[0], dtype=torch.bool)
    s = scores64(q, k, heads)
    A = torch.einsum('hnd,hmd->hnm', ofw._heads(q.double(), heads).abs(), ofw._heads(k.double(), heads).abs()).amax(-1) / 32 ** 0.5
    top = s.topk(keep + 1, dim=-1).values
    return ((top[..., keep - 1] - top[..., keep]) > 2 * 34 * U * A).all(0)


def probabilities(ops, q, k, keep):
    """The kernel's [nq, nk] probabilities for one head's q, k ([n, 32]) -- see the module docstring."""
    nk = k.shape[0]
    H = max(1, -(-nk // 32))
    v = torch.zeros(nk, 32 * H, device='cuda')
    v[torch.arange(nk), torch.arange(nk)] = 1.0
    out = ops.attention(q.cuda().repeat(1, H), k.cuda().repeat(1, H), v, H, keep=keep)
    return out[:, :nk].cpu()


def keeps_for(n):
    return sorted({0, 1, min(n, 2), n // 3, (2 * n) // 3, n - 1, n} - {-1})


@pytest.mark.parametrize('n', SIZES)
def test_selected_set_and_probabilities(ops, n):
    """One head, nq = nk = n: the kernel keeps exactly the fp64 top-k set on every clear row, and its probabilities are the
    fp64 ones within the first-order bound (a probability moves by at most twice its logit's error plus the normaliser's
    n-term sum: (4 (d + 3) A + 4 + 2 n) u, A the largest |logit| contribution -- attention_tolerance with max|v| = 1)."""
    g = torch.Generator().manual_seed(n)
    q, k = torch.randn(n, 32, generator=g), torch.randn(n, 32, generator=g)
    s = scores64(q, k, 1)
    tol = attention_tolerance(q, k, torch.ones(1, 1), 1)
    for keep in keeps_for(n):
        p = probabilities(ops, q, k, keep)
        clear = clear_rows(q, k, 1, keep)
        assert clear.float().mean() > 0.9, (keep, clear.float().mean())
        want_sel = select64(s, keep)[0]
        assert torch.equal(p[clear] != 0, want_sel[clear]), keep
        if keep == 0:
            assert torch.equal(p, torch.zeros_like(p))
            continue
        p64 = torch.where(want_sel, s[0] - s[0].amax(-1, keepdim=True), torch.tensor(-np.inf, dtype=torch.float64)).exp()
        p64 = p64 / p64.sum(-1, keepdim=True)
        assert (p[clear].double() - p64[clear]).abs().max().item() <= tol, keep


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('heads', [1, 4])
def test_output_against_fp64(ops, n, heads):
    """Four heads on padded row strides: the output on every clear row within the first-order fp32 bound of
    test_heads_gpu.attention_tolerance (its argument holds for softmax over a kept subset: the same logits, fewer terms);
    keep = 1 gives exactly the v row of the top key (p = 1, every other product 0); keep = nk is the dense kernel's
    softmax within that bound twice (both are within it of the same fp64 value)."""
    d = 32 * heads
    g = torch.Generator().manual_seed(10 * n + heads)
    q, k, v = (torch.randn(n, d, generator=g) for _ in range(3))
    qd, _ = strided(q, 8)
    kd, _ = strided(k, 4)
    vd, _ = strided(v, 12)
    tol = attention_tolerance(q, k, v, heads)
    s = scores64(q, k, heads)
    for keep in keeps_for(n):
        got = ops.attention(qd, kd, vd, heads, keep=keep).cpu()
        assert got.shape == (n, d)
        clear = clear_rows(q, k, heads, keep)
        want = topk_fp64(q, k, v, heads, keep)
        assert (got[clear].double() - want[clear]).abs().max().item() <= tol, keep
        if keep == 0:
            assert torch.equal(got, torch.zeros_like(got))
        if keep == 1:
            top = s.argmax(-1)  # [heads, n]
            vt = torch.stack([v[top[h], 32 * h:32 * (h + 1)] for h in range(heads)], 1).reshape(n, d)
            assert torch.equal(got[clear], vt[clear])
        if keep == n:
            dense = ops.attention(qd, kd, vd, heads).cpu()
            assert (got.double() - dense.double()).abs().max().item() <= 2 * tol


@pytest.mark.parametrize('n_distinct,copies', [(16, 4), (5, 13), (40, 2)])
def test_ties_keep_the_lowest_indices(ops, n_distinct, copies):
    """Keys in groups of identical rows (interleaved: key j is row j % n_distinct) with different v rows: where `keep`
    cuts a group, the lowest indices of the group are kept -- checked on the read-back selection and on the output."""
    nk = n_distinct * copies
    g = torch.Generator().manual_seed(nk)
    base = torch.randn(n_distinct, 32, generator=g)
    k = base[torch.arange(nk) % n_distinct]
    q = torch.randn(24, 32, generator=g)
    v = torch.randn(nk, 32, generator=g)
    # (scores of the distinct rows, gathered: a BLAS fp64 product of repeated rows is not always bit-equal across them)
    s = scores64(q, base, 1)[..., torch.arange(nk) % n_distinct]
    for keep in range(0, nk + 1, max(1, nk // 23)):
        want = select64(s, keep)[0]
        # rows whose fp64 distinct-score gaps are all clear of the score error (the group order is then certain)
        A = (q.double().abs() @ k.double().abs().T).amax(-1) / 32 ** 0.5
        ds = (q.double() @ base.double().T / 32 ** 0.5).sort(-1).values
        clear = ((ds[:, 1:] - ds[:, :-1]).amin(-1) > 2 * 34 * U * A) if n_distinct > 1 else torch.ones(24, dtype=torch.bool)
        p = probabilities(ops, q, k, keep)
        assert torch.equal(p[clear] != 0, want[clear]), keep
        got = ops.attention(q.cuda(), k.cuda(), v.cuda(), 1, keep=keep).cpu()
        tol = attention_tolerance(q, k, v, 1)
        assert (got[clear].double() - topk_fp64(q, k, v, 1, keep, sel=want[None])[clear]).abs().max().item() <= tol, keep


@pytest.mark.parametrize('n0,n1', [(0, 37), (37, 0), (1, 1), (15, 17), (213, 226), (450, 331), (2100, 300)])
def test_self_pair_is_two_single_calls(ops, n0, n1):
    """Both clouds in one launch with different keep0 / keep1: the bits of two rdm_attention_topk calls (2100: the first
    cloud's scores are formed again per pass, the second's staged in LDS)."""
    heads, d = 4, 128
    n = n0 + n1
    g = torch.Generator().manual_seed(n0 * 7 + n1)
    q, k, v = (torch.randn(n, d, generator=g) for _ in range(3))
    qd, _ = strided(q, 8)
    kd, _ = strided(k, 4)
    vd, _ = strided(v, 12)
    for f0, f1 in ((0.3, 0.7), (1.0, 0.0), (0.57, 1 / 3)):
        keep0, keep1 = ops.topk_count(n0, f0), ops.topk_count(n1, f1)
        got = ops.attention_self_pair(qd, kd, vd, n0, heads, keep=(keep0, keep1))
        for lo, hi, kp in ((0, n0, keep0), (n0, n, keep1)):
            if hi > lo:
                sep = ops.attention(qd[lo:hi], kd[lo:hi], vd[lo:hi], heads, keep=kp)
                assert torch.equal(got[lo:hi], sep), (lo, hi, kp)


def test_bad_arguments_are_refused(ops):
    from rdmnet_amd import _lib
    L = _lib.lib()
    x = torch.zeros(8, 32, device='cuda')
    p = x.data_ptr()
    assert L.rdm_attention_topk(p, 32, p, 32, p, 32, p, 32, 8, 8, 9, 1, 32, None) != 0        # keep > nk
    assert L.rdm_attention_topk(p, 32, p, 32, p, 32, p, 32, 8, 8, -1, 1, 32, None) != 0       # keep < 0
    assert L.rdm_attention_topk(p, 32, p, 32, p, 32, p, 32, 8, 8, 4, 1, 16, None) != 0        # head_dim
    assert L.rdm_attention_topk(p, 30, p, 32, p, 32, p, 32, 8, 8, 4, 1, 32, None) != 0        # unpadded stride
    assert L.rdm_attention_topk(None, 32, p, 32, p, 32, p, 32, 8, 8, 4, 1, 32, None) != 0     # null pointer
    assert L.rdm_attention_self_pair_topk(p, 32, p, 32, p, 32, p, 32, 4, 4, 5, 1, 1, 32, None) != 0  # keep0 > n0
    assert L.rdm_attention_topk(None, 32, None, 32, None, 32, None, 32, 0, 0, 0, 1, 32, None) == 0  # nothing to do
    out = torch.full((5, 32), 7.0, device='cuda')
    assert L.rdm_attention_topk(p, 32, None, 32, None, 32, out.data_ptr(), 32, 5, 0, 0, 1, 32, None) == 0  # nk = 0: zero rows
    assert torch.equal(out.cpu(), torch.zeros(5, 32))


def test_teacher_forced_on_the_reference(ops, golden_dir):
    """The reference's own post-RoPE q, k, v of two top-k self layers (tests/golden/forward_topk_synth0.npz): the kernel keeps
    exactly the reference's selected set (the file records the smallest relative k / k+1 gap of the run, asserted clear of
    the score error below), and its output is the reference's within twice the first-order bound (both are fp32
    evaluations within it of the fp64 value)."""
    import os
    g = np.load(os.path.join(golden_dir, 'forward_topk_synth0.npz'))
    assert g['attn/min_rel_gap'] > 1e-4  # recorded by the generator over every top-k row of the run; derived check below
    for tag in ('l0_ref', 'l2_ref'):
        qh, kh, vh = (torch.from_numpy(g[f'attn/{tag}/{x}']) for x in 'qkv')
        heads, n, _ = qh.shape
        keep = int(g[f'attn/{tag}/keep'])
        flat = lambda t: t.transpose(0, 1).reshape(n, -1).contiguous()
        q, k, v = flat(qh), flat(kh), flat(vh)
        sel = torch.from_numpy(g[f'attn/{tag}/selected'])
        assert clear_rows(q, k, heads, keep).all()  # every row's selection is clear of the score error (derived there)
        assert int(sel[0, 0].sum()) == keep
        for h in range(heads):
            p = probabilities(ops, qh[h], kh[h], keep)
            assert torch.equal(p != 0, sel[h]), (tag, h)
        got = ops.attention(q.cuda(), k.cuda(), v.cuda(), heads, keep=keep).cpu().double()
        ref_out = flat(torch.from_numpy(g[f'attn/{tag}/out'])).double()
        tol = attention_tolerance(q, k, v, heads)
        assert (got - ref_out).abs().max().item() <= 2 * tol, tag
        assert (got - topk_fp64(q, k, v, heads, keep, sel=sel)).abs().max().item() <= tol, tag
