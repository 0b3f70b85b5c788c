"""GPU parity of the head kernels the engine launches on every pair, called through the C-ABI (rdmnet_amd.ops), against
plain float64 CPU restatements: Sinkhorn (every register size class, the 129th "extra line", scattered masks, empty
sides), self-pair attention and the fp32 / bf16 attention kernel at its edges, RoPE, the fused KPConv + GroupNorm, and
the small head kernels (vote shift, sigmoid column, L2 normalisation, index compaction, point-to-node for a pair).
Every tolerance is stated next to its assert with what it is derived from."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import forward as ofw
from test_ops_gpu import kpconv_fp64, padded

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)   # 2^-23: one fp32 ulp at 1
U = EPS / 2                               # fp32 unit roundoff


@pytest.fixture(scope='module')
def ops():
    from rdmnet_amd import ops
    return ops


def strided(t, extra, fill=0.0):
    """[n, c] tensor -> device view whose row stride is c rounded up to 4 plus `extra` floats (the engine's padded ld);
    the bytes outside the view hold `fill`.  Returns (view, backing buffer)."""
    n, c = t.shape
    ld = (c + 3) // 4 * 4 + extra
    buf = torch.full((max(n, 1), ld), fill, dtype=torch.float32, device='cuda')
    buf[:n, :c] = t.cuda()
    return buf[:n, :c], buf


# ----------------------------------------------------------------------------------------------------------- Sinkhorn
COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 67, 68, 69, 99, 100, 101, 127, 128]


def size_class(nr, nc):
    """The register class rdm_sinkhorn picks for a patch: the larger compacted side with the dustbin."""
    side = max(nr, nc) + 1
    for lim, name in ((32, '<=32 (T=8)'), (64, '<=64 (T=4)'), (68, '<=68'), (100, '<=100'), (128, '<=128')):
        if side <= lim:
            return name
    return '129 (extra line)'


def scattered_masks(combos, m, n, g):
    rm, cm = torch.zeros(len(combos), m, dtype=torch.bool), torch.zeros(len(combos), n, dtype=torch.bool)
    for b, (nr, nc) in enumerate(combos):
        rm[b, torch.randperm(m, generator=g)[:nr]] = True
        cm[b, torch.randperm(n, generator=g)[:nc]] = True
    return rm, cm


def run_sinkhorn(ops, scores, rm, cm, alpha, iters):
    """-> (kernel output, fp32 restatement, fp64 restatement), all on the CPU."""
    got = ops.sinkhorn(scores.cuda(), rm.to(torch.uint8).cuda(), cm.to(torch.uint8).cuda(),
                       torch.tensor([alpha], dtype=torch.float32).cuda(), iters).cpu()
    w32 = ofw.sinkhorn(scores, rm, cm, torch.tensor(alpha, dtype=torch.float32), iters)
    w64 = ofw.sinkhorn(scores.double(), rm, cm, torch.tensor(alpha, dtype=torch.float64), iters)
    return got, w32, w64


def sinkhorn_errors(got, w32, w64):
    """Checks a batch entry by entry and returns {entry: (err / max|valid|, the same for the fp32 restatement)}.  Valid
    entries (finite and not masked in the fp64 restatement) against fp64; every other entry -- fl(-1e12), -inf, NaN -- equal
    to the reference's fp32 values."""
    rel = {}
    for b in range(got.shape[0]):
        valid = torch.isfinite(w64[b]) & (w64[b] > -1e11)
        nan = torch.isnan(w32[b])
        assert torch.equal(torch.isnan(got[b]), nan), b
        other = ~valid & ~nan
        assert torch.equal(got[b][other], w32[b][other]), b
        if valid.any():
            scale = w64[b][valid].abs().max().item()
            err = (got[b][valid].double() - w64[b][valid]).abs().max().item()
            err32 = (w32[b][valid].double() - w64[b][valid]).abs().max().item()
            rel[b] = (err / scale, err32 / scale) if scale > 0 else (err, err32)
    return rel


def assert_sinkhorn_bound(rel):
    """The bound of the reference-golden test (tests/test_reference_goldens_gpu.py, test_forward_gpu.py::test_sinkhorn_stage),
    3e-6 of max|valid| per patch -- or twice what the reference's own fp32 arithmetic loses on the patch where that is more.
    The fp32 restatement (bit-exact to the reference's module) misses 3e-6 itself on near-hard assignments (scores of std 60,
    100 iterations: up to 4.8e-6, every size class): its output ((Z + u) + v) - norm rounds at the magnitude of the
    potentials, which exceeds the output's, and the kernel evaluates the same sum in the same order (its error matches the
    restatement's to three digits there)."""
    bad = {b: r for b, r in rel.items() if r[0] > max(SINKHORN_REL, 2 * r[1])}
    assert not bad, bad


SINKHORN_REL = 3e-6   # see assert_sinkhorn_bound


@pytest.mark.parametrize('iters', [0, 1, 100])
@pytest.mark.parametrize('scale,alpha', [(1.0, 1.0), (1.0, -5.0), (1.0, 8.0), (60.0, 1.0), (60.0, -5.0), (60.0, 8.0)])
def test_sinkhorn_every_size_class(ops, iters, scale, alpha):
    """All 16 x 16 valid counts (sides 2 .. 129: every class, both sides of each boundary, the extra row / column) and the
    one-sided extra lines (128, 4) / (4, 128) in ONE batched launch, scattered masks over m = n = 128."""
    combos = list(itertools.product(COUNTS, COUNTS)) + [(128, 4), (4, 128)]
    g = torch.Generator().manual_seed(int(scale) * 1000 + iters * 10 + int(alpha) + 5)
    rm, cm = scattered_masks(combos, 128, 128, g)
    scores = torch.randn(len(combos), 128, 128, generator=g) * scale
    got, w32, w64 = run_sinkhorn(ops, scores, rm, cm, alpha, iters)
    rel = sinkhorn_errors(got, w32, w64)
    worst = {}
    for b, r in rel.items():
        k = size_class(*combos[b])
        worst[k] = max(worst.get(k, (0.0, 0.0)), r)
    print(f'sinkhorn iters={iters} scale={scale} alpha={alpha}: kernel / fp32 reference: '
          + ', '.join(f'{k}: {v[0]:.2e} / {v[1]:.2e}' for k, v in worst.items()))
    assert_sinkhorn_bound(rel)


@pytest.mark.parametrize('m,n', [(77, 128), (128, 77), (128, 33), (5, 128)])
def test_sinkhorn_rectangular_scattered(ops, m, n):
    """m, n other than the valid counts, several classes in one launch (every count that fits each side)."""
    combos = [(r, c) for r in COUNTS for c in COUNTS if r <= m and c <= n] + [(min(m, 4), n), (m, min(n, 4))]
    g = torch.Generator().manual_seed(m * 1000 + n)
    rm, cm = scattered_masks(combos, m, n, g)
    scores = torch.randn(len(combos), m, n, generator=g) * 20
    got, w32, w64 = run_sinkhorn(ops, scores, rm, cm, 1.0, 100)
    assert_sinkhorn_bound(sinkhorn_errors(got, w32, w64))


@pytest.mark.parametrize('iters', [0, 1, 100])
@pytest.mark.parametrize('alpha', [-5.0, 1.0, 8.0])
def test_sinkhorn_empty_sides(ops, iters, alpha):
    """Patches without a valid row, without a valid column, or without either give the reference's outputs
    (tests/test_oracle_sinkhorn.py: -inf dustbin lines, 0.0, NaN) -- bit for bit, since they are exact there -- next to
    ordinary patches in the same launch, which keep the bits they have when launched alone."""
    combos = [(0, 5), (5, 0), (0, 0), (0, 128), (128, 0), (0, 1), (1, 0), (37, 41), (128, 128), (3, 2)]
    g = torch.Generator().manual_seed(iters * 10 + int(alpha) + 5)
    rm, cm = scattered_masks(combos, 128, 128, g)
    scores = torch.randn(len(combos), 128, 128, generator=g) * 5
    got, w32, w64 = run_sinkhorn(ops, scores, rm, cm, alpha, iters)
    # exact where the reference's values are exact: 0.0, -inf, NaN, fl(-1e12) (one empty side after >= 1 iteration, both
    # empty); with iters = 0 a single empty side is the common Z - norm, checked like any patch
    exact = [b for b, (nr, nc) in enumerate(combos) if (nr == 0 or nc == 0) and (iters > 0 or nr + nc == 0)]
    for b in exact:
        nan = torch.isnan(w32[b])
        assert torch.equal(torch.isnan(got[b]), nan), combos[b]
        assert torch.equal(got[b][~nan], w32[b][~nan]), combos[b]
    rest = [b for b in range(len(combos)) if b not in exact]
    assert_sinkhorn_bound(sinkhorn_errors(got[rest], w32[rest], w64[rest]))
    for b in (7, 8, 9):
        alone, _, _ = run_sinkhorn(ops, scores[b:b + 1], rm[b:b + 1], cm[b:b + 1], alpha, iters)
        assert torch.equal(alone[0], got[b])


# ---------------------------------------------------------------------------------------------------------- attention
def dense_fp64(q, k, v, heads, bf16=False):
    """softmax(q k^T / sqrt(d)) v per head ([n, heads * 32] in and out), oracle/forward.py: dense_attention in fp64; bf16:
    the oracle's bf16 form (operands and probabilities rounded to bf16)."""
    h = lambda x: ofw._heads(x.double() if not bf16 else x, heads)
    o = ofw.dense_attention(h(q), h(k), h(v), bf16=bf16)
    return o.double().transpose(0, 1).reshape(q.shape[0], -1)


def attention_tolerance(q, k, v, heads):
    """First-order fp32 error bound of softmax(q k^T / sqrt(d)) v, d = 32: a logit is a d-term dot product, so it is off by at
    most (d + 1) u A with A = max sum_i |q_i k_i| / sqrt(d); the shifted exponentials and the max shift add 2 u A + 2 u, a
    probability moves by twice its logit's error, and the output moves by that times max|v - out| <= 2 max|v|; the two
    nk-term sums (normaliser, P V) add 2 nk u max|v|."""
    d = 32
    qh, kh = ofw._heads(q.double(), heads), ofw._heads(k.double(), heads)
    A = torch.einsum('hnd,hmd->hnm', qh.abs(), kh.abs()).max().item() / d ** 0.5
    vmax = v.abs().max().item()
    return vmax * U * (4 * (d + 3) * A + 4 + 2 * k.shape[0])


@pytest.mark.parametrize('n0,n1', [(0, 37), (37, 0), (1, 1), (15, 17), (16, 48), (47, 49), (200, 3), (431, 411)])
@pytest.mark.parametrize('heads', [1, 4])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('logit', [None, 80.0])
def test_attention_self_pair(ops, n0, n1, heads, bf16, logit):
    """rdm_attention_self_pair against two rdm_attention calls (bit-exact, as the header promises) and fp64 dense
    attention, on views with a padded row stride; logit = 80: q scaled so the largest |logit| of each cloud is 80 (an
    unshifted exp overflows fp32 at 88.7)."""
    d = 32 * heads
    g = torch.Generator().manual_seed(n0 * 1000 + n1 + heads + 7 * bf16)
    n = n0 + n1
    q, k, v = (torch.randn(n, d, generator=g) for _ in range(3))
    if logit is not None:
        for lo, hi in ((0, n0), (n0, n)):
            if hi > lo:
                qh, kh = ofw._heads(q[lo:hi], heads), ofw._heads(k[lo:hi], heads)
                q[lo:hi] *= logit / ((qh @ kh.transpose(1, 2)).abs().max().item() / 32 ** 0.5)
    qd, _ = strided(q, 8)
    kd, _ = strided(k, 4)
    vd, _ = strided(v, 12)
    got = ops.attention_self_pair(qd, kd, vd, n0, heads, bf16=bf16)
    assert got.shape == (n, d)
    for lo, hi in ((0, n0), (n0, n)):
        if hi == lo:
            continue
        sep = ops.attention(qd[lo:hi], kd[lo:hi], vd[lo:hi], heads, bf16=bf16)
        assert torch.equal(got[lo:hi], sep)
        out = got[lo:hi].cpu().double()
        assert torch.isfinite(out).all()
        tol = attention_tolerance(q[lo:hi], k[lo:hi], v[lo:hi], heads)
        if not bf16:
            want = dense_fp64(q[lo:hi], k[lo:hi], v[lo:hi], heads)
            assert (out - want).abs().max().item() <= tol, tol
        else:
            # the oracle's bf16 form: same bf16 operands; it rounds the normalised probabilities, the kernel the ones shifted
            # by its running maximum -- each within 2^-9 relative, so the two differ by <= 2^-8 max|v|, plus fp32 rounding
            want = dense_fp64(q[lo:hi], k[lo:hi], v[lo:hi], heads, bf16=True)
            assert (out - want).abs().max().item() <= 2.0 ** -8 * v[lo:hi].abs().max().item() + tol


# --------------------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize('n', [0, 1, 257])
@pytest.mark.parametrize('d_model', [32, 128, 256])
@pytest.mark.parametrize('with_k', [True, False])
def test_rope_in_place(ops, n, d_model, with_k):
    """rdm_rope rotates q (and k) in place, pair p of row r by 2 pi sigmoid(emb[r, p]), against oracle rotary in fp64, on
    strided views whose padding must not change (k = None: only q rotates)."""
    g = torch.Generator().manual_seed(n * 7 + d_model + with_k)
    q, k = torch.randn(n, d_model, generator=g) * 3, torch.randn(n, d_model, generator=g) * 3
    emb = torch.randn(n, d_model // 2, generator=g) * 4
    qd, qbuf = strided(q, 8, fill=12345.0)
    kd, kbuf = strided(k, 4, fill=-777.0)
    ed, _ = strided(emb, 4)
    q_before, k_before = qbuf.clone(), kbuf.clone()
    ops.rope(qd, kd if with_k else None, ed)
    for x, view, buf, before, rotates in ((q, qd, qbuf, q_before, True), (k, kd, kbuf, k_before, with_k)):
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:n, :d_model] = False
        assert torch.equal(buf[outside], before[outside])          # padding and spare rows untouched
        if not rotates:
            assert torch.equal(buf, before)
            continue
        want = ofw.rotary(x.double()[None], emb.double()[None])[0]
        # theta = 2 pi sigmoid(e) in fp32 is within 4 ulps of 2 pi (16 eps) of the exact angle; cos / sin, the two products
        # and the add add 4 eps: |err| <= 20 eps (|x0| + |x1|) for both entries of a pair
        pair = (x[:, 0::2].abs() + x[:, 1::2].abs()).double().repeat_interleave(2, dim=1)
        err = (view.cpu().double() - want).abs()
        assert (err <= 20 * EPS * pair).all(), (err / pair).max().item() / EPS


# --------------------------------------------------------------------------------------------- fused KPConv + GroupNorm
@pytest.mark.parametrize('c', [1, 32, 64])
@pytest.mark.parametrize('ordered', [False, True])
def test_kpconv_fused_group_norm(ops, c, ordered):
    """rdm_kpconv_fused_group_norm = leaky_relu(GroupNorm_32(KPConv(.))) against fp64 KPConv -> GroupNorm -> leaky ReLU
    (modules.py:141-145, 205-207), with and without order records; conv_out is the same bits either way."""
    cout = 64 if c == 1 else c
    g = torch.Generator().manual_seed(31 * c + ordered)
    ns, m, h = 1500, 1000, 40
    s_pts = torch.randn(ns, 3, generator=g) * 2
    q_pts = s_pts[torch.randint(0, ns, (m,), generator=g)] + 0.1 * torch.randn(m, 3, generator=g)
    feats = torch.randn(ns, c, generator=g) if c > 1 else torch.ones(ns, 1)
    d = torch.cdist(q_pts, s_pts)
    idx = d.argsort(1)[:, :h].contiguous()
    n_valid = torch.randint(0, h + 1, (m,), generator=g)
    n_valid[0] = h
    idx = torch.where(torch.arange(h)[None] < n_valid[:, None], idx, torch.full_like(idx, ns))
    kp = torch.randn(15, 3, generator=g) * 0.3
    W = torch.randn(15, c, cout, generator=g) / np.sqrt(15 * c)
    bias = torch.randn(cout, generator=g)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    sigma = 0.5
    conv_ref = kpconv_fp64(q_pts, s_pts, feats, idx, kp, sigma, W, bias)
    want = F.leaky_relu(F.group_norm(conv_ref.t()[None], 32, gamma.double(), beta.double(), 1e-5)[0].t(), 0.1)
    packed = torch.from_numpy(ops.kpconv_pack_weights(W.numpy())).cuda()
    fd = padded(feats)
    args = (q_pts.cuda(), s_pts.cuda(), fd, ops.row_positive(fd), idx.cuda(), kp.cuda(), sigma, packed, bias.cuda(), cout,
            gamma.cuda(), beta.cuda(), 32)
    perm = torch.argsort(q_pts[:, 0])
    rec = torch.cat([q_pts[perm], perm.to(torch.int32).view(torch.float32)[:, None]], 1).contiguous().cuda()
    y, conv = ops.kpconv_fused_group_norm(*args, order=rec if ordered else None, return_conv=True)
    _, conv_other = ops.kpconv_fused_group_norm(*args, order=None if ordered else rec, return_conv=True)
    assert torch.equal(conv, conv_other)      # the convolution does not depend on the visiting order (rdmnet_hip.h)
    # the KPConv bound of test_ops_gpu.py (2e-5 of the range) ...
    conv_err = (conv.cpu().double() - conv_ref).abs().max().item()
    assert conv_err <= 2e-5 * max(1.0, conv_ref.abs().max().item())
    # ... carried through the normalisation: an input error e moves (x - mean) / std by <= 2 e / std of its group (mean and
    # std move by <= e), times max gamma; plus the fp32 rounding of the normalised value (2e-6 of the output range)
    std = conv_ref.reshape(m, 32, cout // 32).transpose(0, 1).reshape(32, -1).std(1, unbiased=False).min().item()
    tol = 2 * conv_err / std * gamma.max().item() + 2e-6 * want.abs().max().item()
    assert (y.cpu().double() - want).abs().max().item() <= tol


# ---------------------------------------------------------------------------------------------------- small head kernels
@pytest.mark.parametrize('n', [0, 1, 3, 1000])
def test_vote_shift_is_exact(ops, n):
    """xyz + clamp(offset[:, :3], -limit, limit) (vote.py:98-108): one clamp and one fp32 add -> equal to fp32 torch, offsets
    beyond the limits on both sides, offsets read from a strided [n, 8] view."""
    g = torch.Generator().manual_seed(n)
    xyz, off = torch.randn(n, 3, generator=g) * 10, torch.randn(n, 8, generator=g) * 3
    if n:
        off[0, :3] = torch.tensor([100.0, -100.0, 0.25])
    lim = (1.0, 0.5, 2.0)
    got = ops.vote_shift(xyz.cuda(), strided(off, 4)[0], lim)
    want = xyz + torch.maximum(torch.minimum(off[:, :3], torch.tensor(lim)), -torch.tensor(lim))
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('n', [0, 1, 300])
def test_sigmoid_column(ops, n):
    """clamp(sigmoid(x[:, j]), 0, 1) of a strided column, with x = +-100 among the entries."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(max(n, 1), 5, generator=g) * 6
    x[0, 2] = 100.0
    if n > 1:
        x[1, 2] = -100.0
    xd, _ = strided(x, 4)
    got = ops.sigmoid_column(xd[:n, 2]).cpu().double()
    assert got.shape == (n,)
    want = torch.sigmoid(x[:n, 2].double())
    # 1 / (1 + expf(-x)): expf within 2 ulps, add and divide 1 ulp each -> 4 eps relative; below the smallest normal
    # fp32 (sigmoid(-100) = 3.7e-44) the kernel may return 0
    assert ((got - want).abs() <= 4 * EPS * want + np.finfo(np.float32).tiny).all()
    assert torch.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()


@pytest.mark.parametrize('c', [1, 63, 64, 65, 2048])
def test_l2_normalize(ops, c):
    """F.normalize(x, p=2, dim=1) against fp64 on a strided input; an all-zero row gives zeros (norm clamped to 1e-12); no
    rows at all is a no-op."""
    assert ops.l2_normalize(torch.zeros(5, c, device='cuda')[:0]).shape == (0, c)
    n = 37
    g = torch.Generator().manual_seed(c)
    x = torch.randn(n, c, generator=g) * 5
    x[3] = 0.0
    got = ops.l2_normalize(strided(x, 4)[0]).cpu().double()
    want = F.normalize(x.double(), p=2, dim=1)
    assert torch.equal(got[3], torch.zeros(c, dtype=torch.float64))
    # the sum of squares: <= c/64 fp32 adds per lane, a 6-level lane tree, c products -> (c/64 + 7) u relative; the square
    # root halves it, the division adds an ulp: |err| <= (c/64 + 9) eps |y|
    assert ((got - want).abs() <= (c / 64 + 9) * EPS * want.abs()).all()


@pytest.mark.parametrize('kind', ['random', 'all', 'none'])
@pytest.mark.parametrize('begin,end', [(0, 5000), (1000, 4097), (777, 777), (3, 1030)])
def test_compact_indices(ops, kind, begin, end):
    """The kept rows of [begin, end) in ascending order (torch.nonzero of the mask) and their count; nothing is written
    past the count."""
    g = torch.Generator().manual_seed(begin + end)
    keep = {'random': (torch.rand(5000, generator=g) < 0.3), 'all': torch.ones(5000, dtype=torch.bool),
            'none': torch.zeros(5000, dtype=torch.bool)}[kind].to(torch.uint8)
    order = torch.full((5000,), -7, dtype=torch.int32, device='cuda')
    count = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    ops.compact_indices(keep.cuda(), begin, end, order, count)
    want = torch.nonzero(keep[begin:end]).flatten().to(torch.int32) + begin
    c = int(count)
    assert c == want.numel()
    assert torch.equal(order[:c].cpu(), want)
    assert (order[c:] == -7).all()


def test_point_to_node_pair_equals_two_single_calls(ops):
    """Two clouds of different sizes in one set of launches give the two rdm_point_to_node results; a node of the second
    cloud owning more than 4096 points raises the status flag in both forms, the first cloud's call leaves it clear."""
    g = torch.Generator().manual_seed(11)
    pa = torch.randn(3000, 3, generator=g) * 5
    na = pa[torch.randperm(3000, generator=g)[:200]] + 0.01
    pb = torch.cat([torch.randn(4500, 3, generator=g) * 0.1, torch.randn(1200, 3, generator=g) * 5 + 20])
    nb = torch.cat([torch.zeros(1, 3), pb[4500 + torch.randperm(1200, generator=g)[:150]] + 0.01])
    for k in (64, 128):
        st_pair = torch.zeros(1, dtype=torch.int32, device='cuda')
        (a_nm, a_knn, a_km), (b_nm, b_knn, b_km) = ops.point_to_node_pair(pa.cuda(), na.cuda(), pb.cuda(), nb.cuda(), k, st_pair)
        st_a = torch.zeros(1, dtype=torch.int32, device='cuda')
        st_b = torch.zeros(1, dtype=torch.int32, device='cuda')
        sa = ops.point_to_node(pa.cuda(), na.cuda(), k, st_a)
        sb = ops.point_to_node(pb.cuda(), nb.cuda(), k, st_b)
        for got, want in zip((a_nm, a_knn, a_km, b_nm, b_knn, b_km), sa + sb):
            assert torch.equal(got, want)
        assert int(st_a) == 0 and int(st_b) == 1 and int(st_pair) == 1
