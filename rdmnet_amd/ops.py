"""Functional front-end of the C-ABI kernels on torch CUDA tensors (device memory + stream only).

Every function enqueues on the current torch stream and returns freshly allocated outputs.  Feature
matrices are row-major with a row stride that is a multiple of 4 floats (`.stride(0)`); logical
widths are passed explicitly where they differ.  No function here falls back to torch math.
"""
import ctypes
import numbers

import torch

from . import _lib, config

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def pad4(n):
    return (int(n) + 3) // 4 * 4


class Scratch:
    """Grow-only device scratch for kernels that take a caller workspace."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(1 << 24, dtype=torch.uint8, device=device)

    def get(self, nbytes):
        if self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


_scratch = {}


def scratch(device, nbytes):
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    s = _scratch.get(key)
    if s is None:
        s = _scratch[key] = Scratch(device)
    return s.get(nbytes)


def feat_empty(n, c, device):
    """[n, c] view of a buffer whose row stride is padded to a multiple of 4 floats."""
    ld = pad4(c)
    buf = torch.empty((max(int(n), 1), ld), dtype=torch.float32, device=device)
    return buf[:n, :c]


def _ld(t):
    return t.stride(0) if t.dim() == 2 else t.shape[-1]


def gemm(a, b, k, n, *, trans_b=False, bias=None, rowdiv=None, act=ACT_NONE, out=None):
    """out[m, :n] = act(a[m, :k] @ op(b) / rowdiv + bias).  a: [m, >=k] view, b: [k(pad), n(pad)]
    (trans_b False) or [n, >=k] view (trans_b True); k must be a multiple of 4."""
    L = _lib.lib()
    m = a.shape[0]
    if a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError('gemm operands must be row-major (unit column stride)')
    if out is None:
        out = feat_empty(m, n, a.device)
    ws_bytes = L.rdm_gemm_workspace_bytes(m, n, 1)
    ws = scratch(a.device, ws_bytes)
    _lib.check(L.rdm_gemm(a.data_ptr(), _ld(a), 0, b.data_ptr(), _ld(b), 0, int(trans_b), out.data_ptr(), _ld(out),
                          0, m, n, k, 1, _lib.ptr(bias), _lib.ptr(rowdiv), act, ws.data_ptr(), ws.numel(),
                          _lib.stream_ptr()), 'rdm_gemm')
    return out


def gemm_batched(a, b, k, *, trans_b=True, out=None, rowdiv=None):
    """a [B, m, >=k], b [B, n, >=k] contiguous batches -> out [B, m, n] (/ rowdiv[row])."""
    L = _lib.lib()
    B, m, n = a.shape[0], a.shape[1], b.shape[1]
    if out is None:
        out = torch.empty((B, m, n), dtype=torch.float32, device=a.device)
    _lib.check(L.rdm_gemm(a.data_ptr(), a.stride(1), a.stride(0), b.data_ptr(), b.stride(1), b.stride(0),
                          int(trans_b), out.data_ptr(), out.stride(1), out.stride(0), m, n, k, B, 0, _lib.ptr(rowdiv), ACT_NONE, 0, 0,
                          _lib.stream_ptr()), 'rdm_gemm(batched)')
    return out


def patch_scores(ref_feats, ref_idx, src_feats, src_idx, rowdiv=None):
    """scores[b, i, j] = <ref_feats[ref_idx[b, i]], src_feats[src_idx[b, j]]> / rowdiv[i] (model_infer.py:291-311); an index
    outside the tensor selects a zero row.  ref_idx / src_idx: [B, k] int64 -> [B, k, k]."""
    L = _lib.lib()
    B, k = ref_idx.shape
    out = torch.empty((B, k, k), dtype=torch.float32, device=ref_feats.device)
    _lib.check(L.rdm_patch_scores(ref_feats.data_ptr(), _ld(ref_feats), ref_feats.shape[0], ref_idx.data_ptr(), src_feats.data_ptr(),
                                  _ld(src_feats), src_feats.shape[0], src_idx.data_ptr(), B, k, ref_feats.shape[1], _lib.ptr(rowdiv),
                                  out.data_ptr(), _lib.stream_ptr()), 'rdm_patch_scores')
    return out


def row_positive(x):
    L = _lib.lib()
    out = torch.empty((max(x.shape[0], 1),), dtype=torch.uint8, device=x.device)
    _lib.check(L.rdm_row_positive(x.data_ptr(), x.shape[0], x.shape[1], _ld(x), out.data_ptr(), _lib.stream_ptr()),
               'rdm_row_positive')
    return out


def kpconv_gather(q_points, s_points, s_feats, s_positive, idx, kernel_points, sigma, width=None, order=None, form=0):
    """-> (wf [m, pad4(15*c)] view, nn [m]).  order: the query level's cell-sorted records (radius_grid_records) = the order the
    queries are visited in; form: 0 = the library's choice, 1 = one wavefront per (query, slice), 2 = the LDS-tile form (needs
    `order`, c a multiple of 64 >= 128, at most 128 slots).  The same bits in every form and order."""
    L = _lib.lib()
    m, c = q_points.shape[0], s_feats.shape[1]
    kdim = 16 if c == 1 else 15 * c
    wf = feat_empty(m, kdim, q_points.device)
    nn = torch.empty((max(m, 1),), dtype=torch.float32, device=q_points.device)
    _lib.check(L.rdm_kpconv_gather_form(q_points.data_ptr(), m, s_points.data_ptr(), s_points.shape[0], s_feats.data_ptr(),
                                        c, _ld(s_feats), s_positive.data_ptr(), idx.data_ptr(), idx.shape[1], idx.stride(0),
                                        _lib.ptr(width), kernel_points.data_ptr(), float(sigma), wf.data_ptr(), _ld(wf),
                                        nn.data_ptr(), _lib.ptr(order), int(form), _lib.stream_ptr()), 'rdm_kpconv_gather')
    return wf, nn


def kpconv_fused_enabled():
    return bool(_lib.lib().rdm_kpconv_fused_enabled())


def kpconv_fused_supported(c_in, c_out):
    return bool(_lib.lib().rdm_kpconv_fused_supported(int(c_in), int(c_out)))


def kpconv_pack_weights(w):
    """KPConv weights [15, c_in, c_out] (numpy, checkpoint layout) -> float32 numpy array in the fused kernel's operand order."""
    import numpy as np
    L = _lib.lib()
    _, c_in, c_out = w.shape
    w = np.ascontiguousarray(w, dtype=np.float32)
    out = np.empty((L.rdm_kpconv_packed_floats(c_in, c_out),), dtype=np.float32)
    _lib.check(L.rdm_kpconv_pack_weights(w.ctypes.data, c_in, c_out, out.ctypes.data), 'rdm_kpconv_pack_weights')
    return out


def kpconv_fused(q_points, s_points, s_feats, s_positive, idx, kernel_points, sigma, w_packed, bias, c_out, width=None,
                 want_partials=False, order=None, form=0):
    """The whole KPConv.forward (kpconv.py:79-122) in one kernel (c_in = 1, 32, 64) -> out [m, c_out]
    (, fp64 GroupNorm partials [blocks, 2, c_out])."""
    L = _lib.lib()
    m, c = q_points.shape[0], s_feats.shape[1]
    out = feat_empty(m, c_out, q_points.device)
    part = None
    if want_partials:
        nblk = max(int(L.rdm_kpconv_fused_partial_rows(m, c)), 1)
        part = torch.empty((nblk, 2, c_out), dtype=torch.float64, device=q_points.device)
    _lib.check(L.rdm_kpconv_fused_form(q_points.data_ptr(), m, s_points.data_ptr(), s_points.shape[0], s_feats.data_ptr(), c,
                                  _ld(s_feats), s_positive.data_ptr(), idx.data_ptr(), idx.shape[1], idx.stride(0), _lib.ptr(width),
                                  kernel_points.data_ptr(), float(sigma), w_packed.data_ptr(), bias.data_ptr(), c_out,
                                       out.data_ptr(), _ld(out), _lib.ptr(part), _lib.ptr(order), int(form), _lib.stream_ptr()),
               'rdm_kpconv_fused')
    return (out, part) if want_partials else out


def kpconv_fused_group_norm(q_points, s_points, s_feats, s_positive, idx, kernel_points, sigma, w_packed, bias, c_out, gamma,
                            beta, groups, *, width=None, act=ACT_LEAKY, eps=1e-5, order=None, return_conv=False):
    """act(GroupNorm(KPConv(...))) -- the fused convolution followed by the normalisation every backbone block applies.
    return_conv: also return the convolution output the normalisation read -> (y, conv)."""
    L = _lib.lib()
    m, c = q_points.shape[0], s_feats.shape[1]
    conv, y = feat_empty(m, c_out, q_points.device), feat_empty(m, c_out, q_points.device)
    ws = scratch(q_points.device, L.rdm_kpconv_fused_workspace_bytes(m, c, c_out))
    _lib.check(L.rdm_kpconv_fused_group_norm(q_points.data_ptr(), m, s_points.data_ptr(), s_points.shape[0], s_feats.data_ptr(), c,
                                             _ld(s_feats), s_positive.data_ptr(), idx.data_ptr(), idx.shape[1], idx.stride(0),
                                             _lib.ptr(width), kernel_points.data_ptr(), float(sigma), w_packed.data_ptr(),
                                             bias.data_ptr(), c_out, groups, gamma.data_ptr(), beta.data_ptr(), eps, act,
                                             conv.data_ptr(), _ld(conv), y.data_ptr(), _ld(y), ws.data_ptr(), ws.numel(),
                                             _lib.ptr(order), _lib.stream_ptr()), 'rdm_kpconv_fused_group_norm')
    return (y, conv) if return_conv else y


def group_norm(x, gamma, beta, groups, *, act=ACT_NONE, residual=None, want_positive=False, eps=1e-5, form=0):
    """form: 0 = the library's launch structure (finalize + apply as one launch on the coarse levels), 1 = three launches."""
    L = _lib.lib()
    n, c = x.shape
    y = feat_empty(n, c, x.device)
    pos = torch.empty((max(n, 1),), dtype=torch.uint8, device=x.device) if want_positive else None
    ws_bytes = L.rdm_group_norm_workspace_bytes(n, c)
    ws = scratch(x.device, ws_bytes)
    _lib.check(L.rdm_group_norm_form(x.data_ptr(), n, c, _ld(x), groups, gamma.data_ptr(), beta.data_ptr(), eps,
                                     _lib.ptr(residual), _ld(residual) if residual is not None else 0, act, y.data_ptr(),
                                     _ld(y), _lib.ptr(pos), ws.data_ptr(), ws.numel(), int(form), _lib.stream_ptr()), 'rdm_group_norm')
    return (y, pos) if want_positive else y


def linear_group_norm(x, b, k, n, bias, gamma, beta, groups, *, rowdiv=None, act=ACT_NONE, residual=None,
                      want_positive=False, eps=1e-5):
    """act(GroupNorm(x[:, :k] @ b + bias [/ rowdiv]) [+ residual]); statistics from the GEMM epilogue."""
    L = _lib.lib()
    m = x.shape[0]
    lin = feat_empty(m, n, x.device)
    y = feat_empty(m, n, x.device)
    pos = torch.empty((max(m, 1),), dtype=torch.uint8, device=x.device) if want_positive else None
    ws = scratch(x.device, L.rdm_linear_group_norm_workspace_bytes(m, n))
    _lib.check(L.rdm_linear_group_norm(x.data_ptr(), _ld(x), b.data_ptr(), _ld(b), _lib.ptr(bias), _lib.ptr(rowdiv), m, n, k,
                                       groups, gamma.data_ptr(), beta.data_ptr(), eps, _lib.ptr(residual),
                                       _ld(residual) if residual is not None else 0, act, lin.data_ptr(), _ld(lin),
                                       y.data_ptr(), _ld(y), _lib.ptr(pos), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_linear_group_norm')
    return (y, pos) if want_positive else y


def decoder_stage(coarse, idx, skip, b, n, bias, gamma=None, beta=None, groups=32, *, act=ACT_NONE, eps=1e-5):
    """One decoder stage (backbone.py:118-151): act(GroupNorm([coarse[idx[:, 0]] | skip] @ b + bias)), or the plain Linear when
    gamma is None.  b: [pad4(c1 + c2), pad4(n)] as for gemm."""
    L = _lib.lib()
    m, c1, c2 = skip.shape[0], coarse.shape[1], skip.shape[1]
    lin = feat_empty(m, n, skip.device)
    y = feat_empty(m, n, skip.device) if gamma is not None else None
    ws = scratch(skip.device, L.rdm_decoder_stage_workspace_bytes(m, n, c1 + c2))
    _lib.check(L.rdm_decoder_stage(coarse.data_ptr(), coarse.shape[0], c1, _ld(coarse), idx.data_ptr(), _ld(idx), skip.data_ptr(),
                                   c2, _ld(skip), m, b.data_ptr(), _ld(b), _lib.ptr(bias), n, groups, _lib.ptr(gamma),
                                   _lib.ptr(beta), eps, act, lin.data_ptr(), _ld(lin), _lib.ptr(y), _ld(y) if y is not None else 0,
                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_decoder_stage')
    return y if gamma is not None else lin


def layer_norm(x, gamma, beta, *, residual=None, act=ACT_NONE, eps=1e-5, out=None):
    L = _lib.lib()
    n, c = x.shape
    y = out if out is not None else feat_empty(n, c, x.device)
    _lib.check(L.rdm_layer_norm(x.data_ptr(), n, c, _ld(x), _lib.ptr(residual),
                                _ld(residual) if residual is not None else 0, gamma.data_ptr(), beta.data_ptr(), eps,
                                act, y.data_ptr(), _ld(y), _lib.stream_ptr()), 'rdm_layer_norm')
    return y


def attention_tail(hidden, x, wo, bo, gamma1, beta1, w1, b1, w2, b2, gamma2, beta2, *, eps=1e-5, out=None):
    """The tail of an attention layer in one launch: y = LN(hidden @ wo.T + bo + x); out = LN(relu(y @ w1.T + b1) @ w2.T
    + b2 + y).  Width 128, FFN 256; weights as nn.Linear stores them (wo [128,128], w1 [256,128], w2 [128,256])."""
    L = _lib.lib()
    m = hidden.shape[0]
    y = out if out is not None else feat_empty(m, 128, hidden.device)
    _lib.check(L.rdm_attention_tail(hidden.data_ptr(), _ld(hidden), x.data_ptr(), _ld(x), m, wo.shape[0], wo.data_ptr(), _ld(wo),
                                    _lib.ptr(bo), gamma1.data_ptr(), beta1.data_ptr(), w1.data_ptr(), _ld(w1), _lib.ptr(b1),
                                    w2.data_ptr(), _ld(w2), _lib.ptr(b2), gamma2.data_ptr(), beta2.data_ptr(), eps,
                                    y.data_ptr(), _ld(y), _lib.stream_ptr()), 'rdm_attention_tail')
    return y


def attention_tail_pack_weights(wo, w1, w2):
    """wo [128,128], w1 [256,128], w2 [128,256] (nn.Linear layout) -> the tail kernel's operand order (one 81 920-float tensor)."""
    L = _lib.lib()
    packed = torch.empty((L.rdm_attention_tail_packed_floats(),), dtype=torch.float32, device=wo.device)
    _lib.check(L.rdm_attention_tail_pack_weights(wo.data_ptr(), _ld(wo), w1.data_ptr(), _ld(w1), w2.data_ptr(), _ld(w2), packed.data_ptr(),
                                                 _lib.stream_ptr()), 'rdm_attention_tail_pack_weights')
    return packed


def attention_tail_packed(hidden, x, packed, bo, gamma1, beta1, b1, b2, gamma2, beta2, *, eps=1e-5, out=None):
    """attention_tail on weights packed by attention_tail_pack_weights: the same bits, contiguous weight loads."""
    L = _lib.lib()
    m = hidden.shape[0]
    y = out if out is not None else feat_empty(m, 128, hidden.device)
    _lib.check(L.rdm_attention_tail_packed(hidden.data_ptr(), _ld(hidden), x.data_ptr(), _ld(x), m, 128, packed.data_ptr(), _lib.ptr(bo),
                                           gamma1.data_ptr(), beta1.data_ptr(), _lib.ptr(b1), _lib.ptr(b2), gamma2.data_ptr(), beta2.data_ptr(),
                                           eps, y.data_ptr(), _ld(y), _lib.stream_ptr()), 'rdm_attention_tail_packed')
    return y


def linear_layer_norm(x, w, k, n, bias, gamma, beta, *, residual=None, act=ACT_NONE, eps=1e-5, out=None):
    """act(LayerNorm(x[:, :k] @ w.T + bias [+ residual])) in one launch; w = nn.Linear weight [128, k] (n must be 128,
    k a multiple of 16)."""
    L = _lib.lib()
    m = x.shape[0]
    y = out if out is not None else feat_empty(m, n, x.device)
    _lib.check(L.rdm_linear_layer_norm(x.data_ptr(), _ld(x), w.data_ptr(), _ld(w), _lib.ptr(bias), m, n, k, _lib.ptr(residual),
                                       _ld(residual) if residual is not None else 0, gamma.data_ptr(), beta.data_ptr(), eps,
                                       act, y.data_ptr(), _ld(y), _lib.stream_ptr()), 'rdm_linear_layer_norm')
    return y


def gather_max(x, idx, width=None):
    L = _lib.lib()
    m, c = idx.shape[0], x.shape[1]
    y = feat_empty(m, c, x.device)
    _lib.check(L.rdm_gather_max(x.data_ptr(), x.shape[0], c, _ld(x), idx.data_ptr(), m, idx.shape[1], idx.stride(0),
                                _lib.ptr(width), y.data_ptr(), _ld(y), _lib.stream_ptr()), 'rdm_gather_max')
    return y


def upsample_concat(coarse, idx, skip):
    L = _lib.lib()
    m, c1, c2 = skip.shape[0], coarse.shape[1], skip.shape[1]
    y = feat_empty(m, c1 + c2, skip.device)
    _lib.check(L.rdm_upsample_concat(coarse.data_ptr(), coarse.shape[0], c1, _ld(coarse), idx.data_ptr(), idx.stride(0),
                                     skip.data_ptr(), c2, _ld(skip), m, y.data_ptr(), _ld(y), _lib.stream_ptr()),
               'rdm_upsample_concat')
    return y


def gather_rows(x, idx, out=None):
    """out[i] = x[idx[i]] bitwise (any 4-byte-multiple row type); out-of-range index -> zero row.
    x: [n, ...] with contiguous trailing dims (row stride may be padded), idx int64 [m]."""
    L = _lib.lib()
    n, m = x.shape[0], idx.shape[0]
    row_bytes = x[0].numel() * x.element_size() if n > 0 else 0
    tail = tuple(x.shape[1:])
    assert row_bytes % 4 == 0 and (x.stride(0) * x.element_size()) % 4 == 0
    if out is None:
        out = torch.empty((m,) + tail, dtype=x.dtype, device=x.device)
    _lib.check(L.rdm_gather_rows(x.data_ptr(), n, row_bytes // 4, x.stride(0) * x.element_size() // 4, idx.data_ptr(), m,
                                 out.data_ptr(), out.stride(0) * out.element_size() // 4, _lib.stream_ptr()),
               'rdm_gather_rows')
    return out


def rope(q, k, emb):
    L = _lib.lib()
    _lib.check(L.rdm_rope(q.data_ptr(), _ld(q), _lib.ptr(k), _ld(k) if k is not None else 0, emb.data_ptr(), _ld(emb),
                          q.shape[0], q.shape[1], _lib.stream_ptr()), 'rdm_rope')


def topk_count(n, frac):
    """int(n * frac) as the library defines it (rdm_topk_count): the kept count of a top-k attention layer."""
    return _lib.lib().rdm_topk_count(int(n), float(frac))


def attention(q, k, v, heads, out=None, bf16=False, keep=None):
    """softmax(q k^T / sqrt(d)) v per head; keep (0 <= keep <= len(k)): each query keeps only its `keep` largest scores
    (rdm_attention_topk, cfg.thdroformer.k2); None: dense."""
    L = _lib.lib()
    nq, d = q.shape
    if out is None:
        out = feat_empty(nq, d, q.device)
    if keep is not None:
        if bf16:
            raise ValueError('attention: no top-k variant of bf16 attention')
        _lib.check(L.rdm_attention_topk(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                                        nq, k.shape[0], int(keep), heads, d // heads, _lib.stream_ptr()), 'rdm_attention_topk')
        return out
    fn = L.rdm_attention_bf16 if bf16 else L.rdm_attention
    _lib.check(fn(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                               nq, k.shape[0], heads, d // heads, _lib.stream_ptr()), 'rdm_attention')
    return out


def attention_self_pair(q, k, v, n0, heads, out=None, bf16=False, keep=None):
    """Self-attention of two stacked clouds (rows [0, n0) and [n0, n)) in one launch; same results as two attention calls.
    keep = (keep0, keep1): top-k attention, cloud 0 keeping keep0 keys per query and cloud 1 keep1 (rdm_attention_self_pair_topk)."""
    L = _lib.lib()
    n, d = q.shape
    if out is None:
        out = feat_empty(n, d, q.device)
    if keep is not None:
        if bf16:
            raise ValueError('attention_self_pair: no top-k variant of bf16 attention')
        keep0, keep1 = keep
        _lib.check(L.rdm_attention_self_pair_topk(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(),
                                                  _ld(out), n0, n - n0, int(keep0), int(keep1), heads, d // heads, _lib.stream_ptr()),
                   'rdm_attention_self_pair_topk')
        return out
    _lib.check(L.rdm_attention_self_pair(q.data_ptr(), _ld(q), k.data_ptr(), _ld(k), v.data_ptr(), _ld(v), out.data_ptr(), _ld(out),
                                         n0, n - n0, heads, d // heads, int(bf16), _lib.stream_ptr()), 'rdm_attention_self_pair')
    return out


def vote_shift(xyz, offsets, limits):
    L = _lib.lib()
    out = torch.empty_like(xyz)
    _lib.check(L.rdm_vote_shift(xyz.data_ptr(), offsets.data_ptr(), _ld(offsets), xyz.shape[0], float(limits[0]),
                                float(limits[1]), float(limits[2]), out.data_ptr(), _lib.stream_ptr()), 'rdm_vote_shift')
    return out


def sigmoid_column(x_col):
    """clamp(sigmoid(x), 0, 1) of a (possibly strided) single column view [n, 1] or [n]."""
    L = _lib.lib()
    n = x_col.shape[0]
    out = torch.empty((max(n, 1),), dtype=torch.float32, device=x_col.device)
    _lib.check(L.rdm_sigmoid_column(x_col.data_ptr(), x_col.stride(0), n, out.data_ptr(), _lib.stream_ptr()),
               'rdm_sigmoid_column')
    return out[:n]


def l2_normalize(x):
    L = _lib.lib()
    y = feat_empty(x.shape[0], x.shape[1], x.device)
    _lib.check(L.rdm_l2_normalize(x.data_ptr(), _ld(x), x.shape[0], x.shape[1], y.data_ptr(), _ld(y), _lib.stream_ptr()),
               'rdm_l2_normalize')
    return y


def radius_search_device(q, s, q_lengths, s_lengths, radius, width, flags):
    """Truncated radius search entirely on the device.  flags: int32[2] = [max_count, status] (zeroed by
    the caller).  Returns idx [nq, width]; the effective width is min(width, flags[0]) (device value)."""
    L = _lib.lib()
    nq, ns, batch = q.shape[0], s.shape[0], q_lengths.shape[0]
    ws = scratch(q.device, L.rdm_radius_neighbors_workspace_bytes(nq, ns, batch))
    out = torch.empty((max(nq, 1), width), dtype=torch.int64, device=q.device)
    _lib.check(L.rdm_radius_neighbors(q.data_ptr(), nq, s.data_ptr(), ns, q_lengths.data_ptr(), s_lengths.data_ptr(), batch,
                                      float(radius), width, out.data_ptr(), 0, flags.data_ptr(), flags[1:].data_ptr(),
                                      ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_radius_neighbors')
    return out[:nq]


def radius_grid_records(points, lengths, radius):
    """The cell-sorted records {x, y, z, row (int bits)} of the search grid of `points` (stacked clouds, `lengths` int64 on
    the device) for `radius`: float32 [n, 4], in (cloud, cell, row) order -- a function of the points alone.  Used as the
    spatial query order of the KPConv kernels (rdm_kpconv_fused / rdm_kpconv_gather_ordered)."""
    L = _lib.lib()
    n = points.shape[0]
    nbytes = L.rdm_radius_grid_workspace_bytes(n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=points.device)  # (its own allocation: the records are a view of it)
    lengths = lengths.to(device=points.device, dtype=torch.int64).contiguous()
    _lib.check(L.rdm_radius_grid_build(points.data_ptr(), n, lengths.data_ptr(), lengths.shape[0], float(radius), ws.data_ptr(),
                                       nbytes, _lib.stream_ptr()), 'rdm_radius_grid_build')
    rec = L.rdm_radius_grid_records(ws.data_ptr(), nbytes, n)
    off = rec - ws.data_ptr()
    return ws[off:off + 16 * max(n, 1)].view(torch.float32).reshape(-1, 4)[:n]


def grid_subsample_device(points, lengths, voxel, form=0):
    """-> (out_points [n,3] capacity buffer, out_lengths int64[batch]) without synchronising.  form: 0 = kernel form by size,
    1 = one workgroup per cloud, 2 = multi-launch (rdm_grid_subsample_form; same output)."""
    L = _lib.lib()
    n, batch = points.shape[0], lengths.shape[0]
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=points.device)
    out_len = torch.empty((batch,), dtype=torch.int64, device=points.device)
    ws = scratch(points.device, L.rdm_grid_subsample_workspace_bytes(n, batch))
    _lib.check(L.rdm_grid_subsample_form(points.data_ptr(), n, lengths.data_ptr(), batch, float(voxel), out.data_ptr(),
                                         out_len.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(), int(form)),
               'rdm_grid_subsample')
    return out, out_len


def nms(idx, width_dev):
    L = _lib.lib()
    n = idx.shape[0]
    keep = torch.empty((max(n, 1),), dtype=torch.uint8, device=idx.device)
    _lib.check(L.rdm_nms(idx.data_ptr(), n, idx.shape[1], idx.stride(0), _lib.ptr(width_dev), keep.data_ptr(),
                         _lib.stream_ptr()), 'rdm_nms')
    return keep[:n]


def compact_indices(keep, begin, end, order, count):
    L = _lib.lib()
    _lib.check(L.rdm_compact_indices(keep.data_ptr(), begin, end, order.data_ptr(), count.data_ptr(), _lib.stream_ptr()),
               'rdm_compact_indices')


def point_to_node(points, nodes, k, status):
    L = _lib.lib()
    n, m = points.shape[0], nodes.shape[0]
    knn = torch.empty((m, k), dtype=torch.int64, device=points.device)
    kmask = torch.empty((m, k), dtype=torch.uint8, device=points.device)
    nmask = torch.empty((m,), dtype=torch.uint8, device=points.device)
    ws = scratch(points.device, L.rdm_point_to_node_workspace_bytes(n, m))
    _lib.check(L.rdm_point_to_node(points.data_ptr(), n, nodes.data_ptr(), m, k, knn.data_ptr(), kmask.data_ptr(),
                                   nmask.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_point_to_node')
    return nmask, knn, kmask


def point_to_node_pair(points_a, nodes_a, points_b, nodes_b, k, status):
    """point_to_node for the ref (a) and src (b) cloud with one set of launches -> ((nmask, knn, kmask) for a, for b)."""
    L = _lib.lib()
    dev = points_a.device
    outs = []
    for pts, nodes in ((points_a, nodes_a), (points_b, nodes_b)):
        m = nodes.shape[0]
        outs.append((torch.empty((m,), dtype=torch.uint8, device=dev), torch.empty((m, k), dtype=torch.int64, device=dev),
                     torch.empty((m, k), dtype=torch.uint8, device=dev)))
    na, ma, nb, mb = points_a.shape[0], nodes_a.shape[0], points_b.shape[0], nodes_b.shape[0]
    ws = scratch(dev, L.rdm_point_to_node_workspace_bytes(na, ma) + L.rdm_point_to_node_workspace_bytes(nb, mb))
    (nma, knna, kma), (nmb, knnb, kmb) = outs
    _lib.check(L.rdm_point_to_node_pair(points_a.data_ptr(), na, nodes_a.data_ptr(), ma, points_b.data_ptr(), nb, nodes_b.data_ptr(),
                                        mb, k, knna.data_ptr(), kma.data_ptr(), nma.data_ptr(), knnb.data_ptr(), kmb.data_ptr(),
                                        nmb.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_point_to_node_pair')
    return outs


def coarse_matching(scores, ref_mask, src_mask, k, dual=True):
    """scores [m, n] view (overwritten) -> (ref_idx i64[k], src_idx i64[k], scores f32[k], count i32[1])."""
    L = _lib.lib()
    m, n = scores.shape
    dev = scores.device
    ri = torch.empty((k,), dtype=torch.int64, device=dev)
    si = torch.empty((k,), dtype=torch.int64, device=dev)
    sc = torch.empty((k,), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = scratch(dev, L.rdm_coarse_matching_workspace_bytes(m, n))
    _lib.check(L.rdm_coarse_matching(scores.data_ptr(), m, n, _ld(scores), ref_mask.data_ptr(), src_mask.data_ptr(),
                                     int(dual), k, ri.data_ptr(), si.data_ptr(), sc.data_ptr(), cnt.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_coarse_matching')
    return ri, si, sc, cnt


def coarse_matching_features(ref_feats, src_feats, ref_mask, src_mask, k, dual=True):
    """L2-normalised superpoint features [m, d], [n, d] (views) -> (ref_idx i64[k], src_idx i64[k], scores f32[k],
    count i32[1]); the stage is evaluated in fp64 (rdm_coarse_matching_features)."""
    L = _lib.lib()
    (m, d), n = ref_feats.shape, src_feats.shape[0]
    dev = ref_feats.device
    ri = torch.empty((k,), dtype=torch.int64, device=dev)
    si = torch.empty((k,), dtype=torch.int64, device=dev)
    sc = torch.empty((k,), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = scratch(dev, L.rdm_coarse_matching_features_workspace_bytes(m, n))
    _lib.check(L.rdm_coarse_matching_features(ref_feats.data_ptr(), _ld(ref_feats), m, src_feats.data_ptr(), _ld(src_feats), n, d,
                                              ref_mask.data_ptr(), src_mask.data_ptr(), int(dual), k, ri.data_ptr(),
                                              si.data_ptr(), sc.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr()), 'rdm_coarse_matching_features')
    return ri, si, sc, cnt


def sinkhorn(scores, row_mask, col_mask, alpha, iters):
    L = _lib.lib()
    b, m, n = scores.shape
    out = torch.empty((b, m + 1, n + 1), dtype=torch.float32, device=scores.device)
    _lib.check(L.rdm_sinkhorn(scores.data_ptr(), b, m, n, row_mask.data_ptr(), col_mask.data_ptr(), alpha.data_ptr(), iters,
                              out.data_ptr(), _lib.stream_ptr()), 'rdm_sinkhorn')
    return out


def lgr(log_scores, ref_pts, src_pts, ref_mask, src_mask, radius, min_corr, steps, *, topk=1, mutual=False, use_dustbin=True,
        confidence_threshold=0.0, use_global_score=False, correspondence_limit=None, global_scores=None):
    """-> (ref_corr [cap,3], src_corr [cap,3], scores [cap], T [4,4], counts i32[3]) -- counts[0] rows are valid.
    The keyword arguments are cfg.fine_matching's (rdm_lgr_options; config.fine_matching_options checks them); with all of them
    at their defaults the call is rdm_lgr.  log_scores: the Sinkhorn output [b, K+1, K+1] -- without use_dustbin only its
    [K, K] block is read (model_infer.py:319-320), or that block itself, contiguous.  global_scores [b]: with use_global_score."""
    L = _lib.lib()
    b, side = ref_mask.shape
    dev = log_scores.device
    o = config.check_fine_matching(dict(topk=topk, mutual=mutual, use_dustbin=use_dustbin, confidence_threshold=confidence_threshold,
                                        use_global_score=use_global_score, correspondence_limit=correspondence_limit), side,
                                   where='lgr: ')  # (a ValueError names the argument: nothing is truncated to an int here)
    opt = None
    if (o['topk'], o['mutual'], o['use_dustbin'], o['use_global_score'], o['correspondence_limit']) != (1, False, True, False, None):
        opt = _lib.FineMatchingOptions.of(**o)
        cap = L.rdm_lgr_options_capacity(b, side, ctypes.byref(opt))
        if log_scores.dim() != 3 or not log_scores.is_contiguous() or log_scores.shape[1] != log_scores.shape[2]:
            raise ValueError(f'lgr: log_scores must be a contiguous [b, n, n] tensor, got {tuple(log_scores.shape)}')
        if o['use_global_score'] and (global_scores is None or global_scores.dtype != torch.float32 or
                                      not global_scores.is_contiguous() or global_scores.shape[0] < b):
            raise ValueError(f'lgr: use_global_score needs global_scores, contiguous float32 with at least {b} entries')
    else:
        cap = b * 2 * side
    rc = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    sc = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    cs = torch.empty((cap,), dtype=torch.float32, device=dev)
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((3,), dtype=torch.int32, device=dev)
    if opt is None:
        ws = scratch(dev, L.rdm_lgr_workspace_bytes(b))
        _lib.check(L.rdm_lgr(log_scores.data_ptr(), ref_pts.data_ptr(), src_pts.data_ptr(), ref_mask.data_ptr(),
                             src_mask.data_ptr(), b, side, float(radius), int(min_corr), int(steps), rc.data_ptr(), sc.data_ptr(),
                             cs.data_ptr(), T.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   'rdm_lgr')
    else:
        ws = scratch(dev, L.rdm_lgr_options_workspace_bytes(b, side, ctypes.byref(opt)))
        _lib.check(L.rdm_lgr_options(log_scores.data_ptr(), log_scores.shape[1], ref_pts.data_ptr(), src_pts.data_ptr(),
                                     ref_mask.data_ptr(), src_mask.data_ptr(), _lib.ptr(global_scores if o['use_global_score'] else None),
                                     b, side, float(radius), int(min_corr), int(steps), ctypes.byref(opt), rc.data_ptr(),
                                     sc.data_ptr(), cs.data_ptr(), T.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr()), 'rdm_lgr_options')
    return rc, sc, cs, T, counts


def voxel_downsample(points, voxel):
    """Raw-scan preprocessing (preporcess/downsample_pcd_kitti.py:21-36): points f32 [N, C>=3] on the GPU ->
    per-voxel means [M, C] (all columns averaged, e.g. xyz + intensity), voxels in first-occurrence order."""
    L = _lib.lib()
    assert points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
    n, c = points.shape
    assert n == 0 or points.stride(1) == 1
    ld = points.stride(0) if n > 1 else c
    out = torch.empty((max(n, 1), c), dtype=torch.float32, device=points.device)
    flags = torch.zeros((2,), dtype=torch.int32, device=points.device)  # [count, status]
    ws = scratch(points.device, L.rdm_voxel_downsample_workspace_bytes(n))
    _lib.check(L.rdm_voxel_downsample(points.data_ptr(), n, ld, c, float(voxel), out.data_ptr(), c,
                                      flags.data_ptr(), flags[1:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_voxel_downsample')
    m, status = (int(x) for x in flags.cpu())  # the output size is data dependent: one read-back
    if status != 0:
        raise RuntimeError('rdm_voxel_downsample: non-finite point or extent beyond 2^21 voxels')
    return out[:m]


def ransac_correspondences(src_corr, ref_corr, distance_threshold=0.3, ransac_n=4, num_iterations=50000, seed=0,
                           return_hypotheses=False):
    """geotransformer/utils/open3d.py:173-203 on the GPU: -> (transform [4,4] f32 device, stats int32[2] device =
    {winning iteration, inliers}, inlier rmse f32[1] device[, per-iteration inlier counts])."""
    L = _lib.lib()
    assert src_corr.is_cuda and src_corr.dtype == torch.float32 and src_corr.is_contiguous() and ref_corr.is_contiguous()
    dev = src_corr.device
    T = torch.empty((4, 4), dtype=torch.float32, device=dev)
    stats = torch.empty((2,), dtype=torch.int32, device=dev)
    rmse = torch.empty((1,), dtype=torch.float32, device=dev)
    hyp = torch.empty((num_iterations,), dtype=torch.int32, device=dev) if return_hypotheses else None
    ws = scratch(dev, L.rdm_ransac_workspace_bytes(num_iterations))
    _lib.check(L.rdm_ransac_correspondences(src_corr.data_ptr(), ref_corr.data_ptr(), src_corr.shape[0], float(distance_threshold),
                                            ransac_n, num_iterations, int(seed), T.data_ptr(), stats.data_ptr(), rmse.data_ptr(),
                                            _lib.ptr(hyp), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_ransac_correspondences')
    return (T, stats, rmse, hyp) if return_hypotheses else (T, stats, rmse)


class RobustResult:
    """rdm_robust_registration's outputs on the host: transformation (float64 [4, 4] numpy, src -> ref, bottom row 0 0 0 1),
    selected (int64 numpy [K]: the rows the pose was estimated from, ascending), the stats by name (num_selected, valid, exact,
    iterations, translation_inliers, edges) and, when asked for, weights (float64 numpy [K (K - 1) / 2]: the final GNC weight
    of pair (p, q) of the selected rows at p K - p (p + 1) / 2 + q - p - 1), degree and core (int32 numpy [C])."""

    def __init__(self, transformation, selected, stats, weights=None, degree=None, core=None):
        self.transformation, self.selected, self.weights, self.degree, self.core = transformation, selected, weights, degree, core
        for name, v in zip(_lib.ROBUST_STATS, stats):
            setattr(self, name, int(v))

    def __repr__(self):
        return (f'RobustResult(num_selected={self.num_selected}, valid={self.valid}, exact={self.exact}, '
                f'iterations={self.iterations}, translation_inliers={self.translation_inliers}, edges={self.edges})')


def robust_registration(src_corr, ref_corr, noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12,
                        inlier_selection='clique', max_clique_nodes=None, return_weights=False, return_graph=False):
    """Outlier-robust pose from correspondences (rdm_robust_registration; DESIGN.md section 7: compatibility graph, maximum
    clique, GNC-TLS rotation, truncated-least-squares translation -- the estimator experiments/eval.py:198-219 names `teaser`,
    this project's own definition).  src_corr / ref_corr: float32 CUDA [C, 3], C <= 16384, the pose moves src onto ref; the
    defaults are eval.py:199-206's.  inlier_selection: 'clique', 'kcore' or 'none'; max_clique_nodes: search nodes per
    subproblem (None: the library's default).  -> RobustResult (the call ends with the read-back of its results)."""
    import numpy as np
    L = _lib.lib()
    for t, name in ((src_corr, 'src_corr'), (ref_corr, 'ref_corr')):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3):
            raise ValueError(f'{name} must be a float32 CUDA tensor [C, 3]')
    if src_corr.shape != ref_corr.shape or src_corr.device != ref_corr.device:
        raise ValueError('src_corr and ref_corr must have the same shape and device')
    if inlier_selection not in _lib.ROBUST_SELECTIONS:
        raise ValueError(f"inlier_selection must be one of {', '.join(_lib.ROBUST_SELECTIONS)}, got {inlier_selection!r}")
    if not (noise_bound > 0 and cbar2 > 0 and gnc_factor > 1 and int(max_iterations) >= 1 and cost_threshold >= 0):
        raise ValueError('noise_bound and cbar2 must be > 0, gnc_factor > 1, max_iterations >= 1, cost_threshold >= 0')
    if max_clique_nodes is not None and int(max_clique_nodes) < 1:
        raise ValueError(f'max_clique_nodes must be >= 1 (or None for the default), got {max_clique_nodes}')
    src_corr, ref_corr = src_corr.contiguous(), ref_corr.contiguous()
    C, dev = src_corr.shape[0], src_corr.device
    mode = _lib.ROBUST_SELECTIONS[inlier_selection]
    n_stats = len(_lib.ROBUST_STATS)
    # transform f64[16], then int32: stats, selected[C], degree[C], core[C] -- one read-back
    out = torch.empty((16 * 2 + n_stats + 3 * C + 2,), dtype=torch.int32, device=dev)
    ints = out[32:]
    stats, selected, degree, core = ints[:n_stats], ints[n_stats:n_stats + C], ints[n_stats + C:n_stats + 2 * C], ints[n_stats + 2 * C:]
    cap = C * (C - 1) // 2 if return_weights else 0
    weights = torch.zeros((max(cap, 1),), dtype=torch.float64, device=dev) if return_weights else None
    ws_bytes = L.rdm_robust_registration_workspace_bytes(min(C, _lib.ROBUST_MAX_CORR), mode)
    ws = scratch(dev, ws_bytes)
    _lib.check(L.rdm_robust_registration(src_corr.data_ptr(), ref_corr.data_ptr(), C, float(noise_bound), float(cbar2),
                                         float(gnc_factor), int(max_iterations), float(cost_threshold), mode,
                                         0 if max_clique_nodes is None else int(max_clique_nodes), out.data_ptr(), stats.data_ptr(),
                                         selected.data_ptr(), _lib.ptr(weights), cap, degree.data_ptr(), core.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_robust_registration')
    host = out.cpu().numpy()
    st = host[32:32 + n_stats]
    K = int(st[0])
    hi = host[32 + n_stats:]
    w = None
    if return_weights:
        w = weights[:K * (K - 1) // 2].cpu().numpy() if st[1] else np.zeros(0)
    return RobustResult(host[:32].view(np.float64).reshape(4, 4).copy(), hi[:K].astype(np.int64), st, w,
                        hi[C:2 * C].copy() if return_graph else None, hi[2 * C:3 * C].copy() if return_graph else None)


# ---- loop-closure detection: Scan Context (rdm_scan_context, rdm_scan_context_distance) ------------------------------------

SCAN_CONTEXT_DEFAULTS = dict(n_rings=20, n_sectors=60, max_range=80.0, lidar_height=2.0)


def _sc_dims(n_rings, n_sectors):
    n_rings, n_sectors = int(n_rings), int(n_sectors)
    if not (1 <= n_rings <= _lib.SCAN_CONTEXT_MAX_DIM and 1 <= n_sectors <= _lib.SCAN_CONTEXT_MAX_DIM):
        raise ValueError(f'n_rings and n_sectors must be 1 ... {_lib.SCAN_CONTEXT_MAX_DIM}, got {n_rings} and {n_sectors}')
    return n_rings, n_sectors


def scan_context(clouds, offsets=None, *, n_rings=20, n_sectors=60, max_range=80.0, lidar_height=2.0, return_normalised=False):
    """Scan Context place descriptors (rdm_scan_context) of a batch of clouds.  clouds: a list of float32
    CUDA tensors [N_i, >=3] (empty ones allowed), or one packed float32 CUDA tensor [N, ld >= 3] with `offsets` (int64
    [n + 1], host or device: cloud i is rows offsets[i] .. offsets[i + 1]).  -> float32 CUDA [n, n_rings, n_sectors]; with
    return_normalised also the column-normalised form float32 [n, n_rings, 64] and the valid-column masks int64 [n] (bit j =
    column j has a point).  A bin is the maximum z + lidar_height of its points and does not depend on their order.  The
    packed form with device offsets enqueues two launches and nothing else; the list form first concatenates the clouds' xyz
    columns on the device (one extra copy of all points; a single cloud is used as it is) and copies the host-built offsets to
    the device, as host offsets in the packed form are.  The stream is never waited for."""
    L = _lib.lib()
    n_rings, n_sectors = _sc_dims(n_rings, n_sectors)
    if not (float(max_range) > 0 and float(max_range) < float('inf')):
        raise ValueError(f'max_range must be positive and finite, got {max_range}')
    if offsets is None:
        if not isinstance(clouds, (list, tuple)):
            raise ValueError('scan_context: clouds must be a list of tensors, or a packed tensor with offsets')
        for i, t in enumerate(clouds):
            _points_arg(t, f'clouds[{i}]')
        if len({t.device for t in clouds}) > 1:
            raise ValueError('scan_context: the clouds are on different devices')
        if not clouds:
            raise ValueError('scan_context: an empty list of clouds has no device; pass a packed tensor with offsets')
        counts = [int(t.shape[0]) for t in clouds]
        points = clouds[0] if len(clouds) == 1 else torch.cat([t[:, :3] for t in clouds])
        offsets = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
    else:
        points = clouds
        _points_arg(points, 'clouds')
        if not (isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 1):
            raise ValueError('offsets must be an int64 tensor [n + 1]')
    dev = points.device
    n = offsets.numel() - 1
    if n > 65535:
        raise ValueError(f'scan_context: {n} clouds, a call takes at most 65535')
    offsets = offsets.to(dev).contiguous()
    ld = points.stride(0) if points.shape[0] > 1 else points.shape[1]
    desc = torch.empty((n, n_rings, n_sectors), dtype=torch.float32, device=dev)
    norm = torch.empty((n, n_rings, _lib.SCAN_CONTEXT_LD), dtype=torch.float32, device=dev) if return_normalised else None
    valid = torch.empty((n,), dtype=torch.int64, device=dev) if return_normalised else None
    with torch.cuda.device(dev):
        ws = scratch(dev, L.rdm_scan_context_workspace_bytes(n, n_rings, n_sectors))
        _lib.check(L.rdm_scan_context(points.data_ptr(), ld, points.shape[0], offsets.data_ptr(), n, n_rings, n_sectors,
                                      float(max_range), float(lidar_height), desc.data_ptr(), _lib.ptr(norm), _lib.ptr(valid),
                                      ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_scan_context')
    return (desc, norm, valid) if return_normalised else desc


class ScanContextSearch:
    """rdm_scan_context_distance's outputs, CUDA tensors: per query `distance` (float32 [n_q]), `index` (int32: the eligible
    candidate of lowest distance, the lowest among equals; -1 without one, then distance = +inf) and `shift` (int32: that
    candidate's column shift; -1); with full=True also `distances` (float32 [n_q, n_c]) and `shifts` (int32 [n_q, n_c]) of every
    pair, eligible or not."""

    def __init__(self, distance, index, shift, distances=None, shifts=None):
        self.distance, self.index, self.shift, self.distances, self.shifts = distance, index, shift, distances, shifts

    def __repr__(self):
        return f'ScanContextSearch(queries={self.distance.shape[0]}, full={self.distances is not None})'


def _sc_desc(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
        raise ValueError(f'{name} must be a float32 CUDA tensor [n, n_rings, n_sectors]')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return t


def scan_context_distance(q_desc, c_desc, *, q_base=0, c_base=0, exclude_recent=50, full=False):
    """Exhaustive Scan Context search (rdm_scan_context_distance): every query descriptor against every candidate under every
    column shift.  q_desc / c_desc: float32 CUDA [n_q | n_c, n_rings, n_sectors] (ops.scan_context).  Query i is frame q_base +
    i, candidate j frame c_base + j; j is eligible for i iff (q_base + i) - (c_base + j) >= exclude_recent (negative: all
    are).  -> ScanContextSearch.  No synchronisation."""
    L = _lib.lib()
    q_desc, c_desc = _sc_desc(q_desc, 'q_desc'), _sc_desc(c_desc, 'c_desc')
    if q_desc.device != c_desc.device or q_desc.shape[1:] != c_desc.shape[1:]:
        raise ValueError(f'scan_context_distance: q_desc {tuple(q_desc.shape)} on {q_desc.device} against c_desc '
                         f'{tuple(c_desc.shape)} on {c_desc.device}')
    n_rings, n_sectors = _sc_dims(q_desc.shape[1], q_desc.shape[2])
    dev, n_q, n_c = q_desc.device, q_desc.shape[0], c_desc.shape[0]
    best = torch.empty((3, max(n_q, 1)), dtype=torch.int32, device=dev)  # distance bits, index, shift
    distance, index, shift = best[0, :n_q].view(torch.float32), best[1, :n_q], best[2, :n_q]
    dists = torch.empty((n_q, n_c), dtype=torch.float32, device=dev) if full else None
    shifts = torch.empty((n_q, n_c), dtype=torch.int32, device=dev) if full else None
    with torch.cuda.device(dev):
        nbytes = L.rdm_scan_context_distance_workspace_bytes(n_q, n_c, n_rings, n_sectors)
        if nbytes == 0:
            raise ValueError(f'scan_context_distance: {n_c} candidates, a call takes at most 2^26')
        ws = scratch(dev, nbytes)
        _lib.check(L.rdm_scan_context_distance(q_desc.data_ptr(), n_q, c_desc.data_ptr(), n_c, n_rings, n_sectors, int(q_base),
                                               int(c_base), int(exclude_recent), distance.data_ptr(), index.data_ptr(),
                                               shift.data_ptr(), _lib.ptr(dists), _lib.ptr(shifts), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr()), 'rdm_scan_context_distance')
    return ScanContextSearch(distance, index, shift, dists, shifts)


def detect_loops(descriptors, threshold=0.13, exclude_recent=50):
    """Loop closures of one sequence: every descriptor (float32 CUDA [n, n_rings, n_sectors], frame order) against every
    earlier one that is at least `exclude_recent` frames older; a loop is accepted iff its distance < threshold.  -> host
    arrays (query int64, candidate int64, distance float32, shift int64, yaw_deg float64), in query order; yaw_deg = shift x 360
    / n_sectors is the rotation about z that takes the candidate scan to the query scan.  One read-back."""
    import numpy as np
    res = scan_context_distance(descriptors, descriptors, exclude_recent=exclude_recent)
    host = torch.stack([res.distance.view(torch.int32), res.index, res.shift]).cpu().numpy()
    dist, index, shift = host[0].view(np.float32), host[1].astype(np.int64), host[2].astype(np.int64)
    query = np.nonzero((index >= 0) & (dist.astype(np.float64) < float(threshold)))[0].astype(np.int64)
    return (query, index[query], dist[query].copy(), shift[query], shift[query] * (360.0 / descriptors.shape[2]))


# ---- voxel map: the scans of a sequence fused under its trajectory (rdm_voxel_map_*) ----------------------------------------

class VoxelMap:
    """A persistent voxel map in world coordinates on the GPU (rdm_voxel_map_*): scans are moved by their
    poses and fused into per-voxel means.  voxel: edge in metres (cell c covers [c voxel, (c + 1) voxel), anchored at the world
    origin); channels C = 3 ... 8: xyz and C - 3 attributes (4: intensity); capacity: the table's first size, a power of two >= 64
    -- it grows by itself.  Per voxel a count and C int64 sums of 20-bit fixed-point values under integer atomic adds, so the
    map depends on the set of integrated points only: the order of the scans, the batching and the run do not change one bit
    of what `extract` returns.  moments=True keeps nine more int64 sums per voxel in a second block (rdm_voxel_moments_*: the first
    and second moments of the 12-bit local coordinates), which give every voxel a mean, a covariance and a normal --
    `extract_moments` -- and the map a sharpness report -- `sharpness`; `extract` and `stats` are the same bytes either way.
    observations=True keeps, in a third block (rdm_voxel_observations_*), in how many distinct scans every voxel was seen and the first and
    the last of them -- `extract_observations` -- and gives the map without the voxels seen in too few scans -- `pruned`: a moving
    object is in a voxel in one scan, a wall in many.  The scans are numbered from 0 as `integrate` is given them, empty ones included
    (`num_scans`: the next id), so a scan must come whole in one `integrate` call.  Again `extract` and `stats` are the same bytes.
    The integers are all a map is: `state` reads them, `from_state` / `save` / `load` rebuild the map from them bit for bit at any
    capacity, and `merge` adds the map of other scans into this one (rdm_voxel_map_export / rdm_voxel_map_import)."""

    def __init__(self, voxel, channels=4, capacity=1 << 20, device='cuda', moments=False, observations=False):
        voxel, channels, capacity = float(voxel), int(channels), int(capacity)
        if not (voxel > 0 and voxel < float('inf')):
            raise ValueError(f'voxel must be positive and finite, got {voxel}')
        if not 3 <= channels <= _lib.VOXEL_MAP_MAX_CHANNELS:
            raise ValueError(f'channels must be 3 ... {_lib.VOXEL_MAP_MAX_CHANNELS}, got {channels}')
        if capacity < 64 or capacity & (capacity - 1) or _lib.lib().rdm_voxel_map_bytes(capacity, channels) == 0:
            raise ValueError(f'capacity must be a power of two in [64, 2^30], got {capacity}')
        self.voxel, self.channels = voxel, channels
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError(f'VoxelMap needs a CUDA device, got {self.device}')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.moments, self.observations = bool(moments), bool(observations)
        self.capacity, self._mom, self._obs = capacity, None, None
        for attr, kind in self._owned():
            setattr(self, attr, self._alloc(kind, capacity))
        self.reset()

    def _owned(self):
        """The blocks this map keeps, in the order of their launches on the stream: (attribute, kind), kind being what stands behind
        `rdm_voxel_` in the names of the block's bytes, reset and rehash entry points."""
        return [('_buf', 'map')] + [('_mom', 'moments')] * self.moments + [('_obs', 'observations')] * self.observations

    def _shape(self, kind, capacity):
        """What the bytes and reset entry points of a block take as its shape."""
        return (capacity, self.channels) if kind == 'map' else (capacity,)

    def _alloc(self, kind, capacity):
        nbytes = getattr(_lib.lib(), f'rdm_voxel_{kind}_bytes')(*self._shape(kind, capacity))
        return torch.empty((nbytes,), dtype=torch.uint8, device=self.device)

    def _head(self):
        return self._buf.data_ptr(), self._buf.numel(), self.capacity, self.channels

    def _rehash_beside(self, kind, old, was, new, now):
        """rdm_voxel_{kind}_rehash: the moments or observations `was` beside the map old = (pointer, bytes, capacity) into `now` beside
        the map `new`, which holds the keys already."""
        name = f'rdm_voxel_{kind}_rehash'
        _lib.check(getattr(_lib.lib(), name)(*old, was.data_ptr(), was.numel(), *new, now.data_ptr(), now.numel(), self.channels,
                                             _lib.stream_ptr()), name)

    def reset(self):
        with torch.cuda.device(self.device):
            for attr, kind in self._owned():
                t, name = getattr(self, attr), f'rdm_voxel_{kind}_reset'
                _lib.check(getattr(_lib.lib(), name)(t.data_ptr(), t.numel(), *self._shape(kind, self.capacity), _lib.stream_ptr()), name)
        self.num_scans = 0  # with observations: the id of the next scan
        self._bound = 0  # occupied <= _bound: spares the read-back of `occupied` while the table is certainly large enough

    def stats(self):
        """{occupied, integrated, skipped_nonfinite, skipped_range, out_of_extent, dropped_full}; waits for the stream."""
        host = (ctypes.c_uint64 * len(_lib.VOXEL_MAP_STATS))()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rdm_voxel_map_stats(*self._head(), ctypes.addressof(host), _lib.stream_ptr()), 'rdm_voxel_map_stats')
        out = dict(zip(_lib.VOXEL_MAP_STATS, (int(v) for v in host)))
        self._bound = out['occupied']
        return out

    def __len__(self):
        return self.stats()['occupied']

    def _reserve(self, n_points):
        """capacity >= 2 (occupied + the batch's points) before a batch, so that through this class nothing is ever dropped."""
        if 2 * (self._bound + n_points) > self.capacity:
            need = 2 * (self.stats()['occupied'] + n_points)
            if need > self.capacity:
                capacity = self.capacity
                while capacity < need:
                    capacity *= 2
                if _lib.lib().rdm_voxel_map_bytes(capacity, self.channels) == 0:
                    raise RuntimeError(f'VoxelMap: {need // 2} voxels need more than 2^30 slots')
                grown = {attr: self._alloc(kind, capacity) for attr, kind in self._owned()}
                old, new = (self._buf.data_ptr(), self._buf.numel(), self.capacity), (grown['_buf'].data_ptr(), grown['_buf'].numel(), capacity)
                with torch.cuda.device(self.device):
                    _lib.check(_lib.lib().rdm_voxel_map_rehash(*old, *new, self.channels, _lib.stream_ptr()), 'rdm_voxel_map_rehash')
                    for attr, kind in self._owned()[1:]:
                        self._rehash_beside(kind, old, getattr(self, attr), new, grown[attr])
                self.capacity = capacity
                self.__dict__.update(grown)  # (the old blocks are freed in stream order by the caching allocator)
        self._bound += n_points

    def _packed(self, what, clouds, poses, min_range, max_range):
        """The argument checks of integrate and register -> (points or None, offsets, n, poses float64 numpy [n, 4, 4], lo, hi)."""
        import numpy as np
        C = self.channels
        if isinstance(clouds, tuple) and len(clouds) == 2 and isinstance(clouds[1], torch.Tensor) and clouds[1].dtype == torch.int64:
            points, offsets = clouds
            if not (offsets.dim() == 1 and offsets.numel() >= 1):
                raise ValueError('offsets must be an int64 tensor [n + 1]')
            named = [(points, 'points')]
        elif isinstance(clouds, (list, tuple)):
            named = [(t, f'clouds[{i}]') for i, t in enumerate(clouds)]
            points = offsets = None
        else:
            raise ValueError(f'VoxelMap.{what}: clouds must be a list of tensors, or (points, offsets)')
        for t, name in named:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= C):
                raise ValueError(f'{name} must be a float32 CUDA tensor [N, >={C}] (the map has {C} channels)')
            if t.shape[0] > 0 and t.stride(1) != 1:
                raise ValueError(f'{name} must have unit column stride')
            if t.device != self.device:
                raise ValueError(f'{name} is on {t.device}, the map on {self.device}')
        if offsets is None:
            counts = [int(t.shape[0]) for t, _ in named]
            offsets = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
            if len(named) == 1:
                points = named[0][0]
            elif named:
                points = torch.cat([t[:, :C] for t, _ in named])
        n = offsets.numel() - 1
        X = self._poses_arg(poses, n, 'scan')
        lo, hi = float(min_range), float(max_range)
        if not 0.0 <= lo <= hi:
            raise ValueError(f'need 0 <= min_range <= max_range, got {min_range} and {max_range}')
        return points, offsets, n, X, lo, hi

    @staticmethod
    def _poses_arg(poses, n, per):
        """poses, anything numpy or torch holds -> float64 numpy [n, 4, 4], finite (per: what a pose belongs to, for the message)."""
        import numpy as np
        if isinstance(poses, torch.Tensor):
            poses = poses.detach().cpu().numpy()
        X = np.ascontiguousarray(np.asarray(poses, dtype=np.float64))
        if X.shape == (4, 4) and n == 1:
            X = X[None]
        if X.size == 0 and n == 0:
            X = X.reshape(0, 4, 4)
        if X.shape != (n, 4, 4):
            raise ValueError(f'poses must be [{n}, 4, 4] (one 4x4 per {per}), got {X.shape}')
        if not np.isfinite(X).all():
            raise ValueError('poses must be finite')
        return X

    @staticmethod
    def _options(sigma, neighbors, rest_ok, rest):
        """The checks of sigma and neighbors that register, align and query share, then the caller's own bounds (rest: their text)."""
        if not (sigma > 0 and sigma < float('inf')):
            raise ValueError(f'sigma must be positive and finite, got {sigma}')
        if neighbors not in (1, 7):
            raise ValueError(f'neighbors must be 1 or 7, got {neighbors}')
        if not rest_ok:
            raise ValueError('need ' + rest)

    def _gauss_newton(self, n, weighted, workspace_bytes, call):
        """The outputs of register and align for n scans or sources: allocates them and, for n > 0, the workspace of the size that the
        entry point `workspace_bytes` names, lets call((transforms, hessians, gradients, costs pointers), weight_sum pointer or None,
        (stats, workspace, its size, stream)) make the C call, and wraps them -> MapRegistrationResult."""
        L, dev = _lib.lib(), self.device
        real = torch.zeros((n, 59), dtype=torch.float64, device=dev)  # transforms, hessians, gradients, costs
        stats = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        T, H, g, cost = (real.view(-1)[a * n:b * n].view(n, b - a) for a, b in ((0, 16), (16, 52), (52, 58), (58, 59)))
        weight_sum = torch.zeros((n,), dtype=torch.float64, device=dev) if weighted else None
        if n > 0:
            with torch.cuda.device(dev):
                ws = scratch(dev, getattr(L, workspace_bytes)(n))
                call((T.data_ptr(), H.data_ptr(), g.data_ptr(), cost.data_ptr()), _lib.ptr(weight_sum),
                     (stats.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return MapRegistrationResult(T.view(n, 4, 4), H.view(n, 6, 6), g, cost.view(n), stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3],
                                     weight_sum)

    def _on_device(self, points, offsets, X):
        """_packed's points, offsets and poses as the C calls take them -> (points, ld, total, offsets and poses on the device).  A batch
        without rows gets one placeholder row and total = 0."""
        if points is None or points.shape[0] == 0:
            points, total, ld = torch.zeros((1, self.channels), dtype=torch.float32, device=self.device), 0, self.channels
        else:
            total = int(points.shape[0])
            ld = points.stride(0) if total > 1 else points.shape[1]
        with torch.cuda.device(self.device):
            return points, ld, total, offsets.to(self.device).contiguous(), torch.from_numpy(X).to(self.device)

    def integrate(self, clouds, poses, min_range=0.0, max_range=float('inf')):
        """clouds: a list of float32 CUDA tensors [N_i, >= C] (empty ones allowed), or a pair (points float32 CUDA [N, ld >= C],
        offsets int64 [n + 1], host or device: scan i is rows offsets[i] .. offsets[i + 1]).  poses: [n, 4, 4] finite, anything
        numpy or torch holds (world = pose @ point).  A point is integrated iff its C values are finite and min_range <= its range
        in the sensor frame <= max_range.  -> self.  The list form concatenates the clouds' first C columns on the device.  With
        observations the scans get the ids num_scans, num_scans + 1, ... (an empty scan consumes one) and a longer batch goes in calls
        of 64 scans, which read the same device arrays."""
        points, offsets, n, X, lo, hi = self._packed('integrate', clouds, poses, min_range, max_range)
        if n == 0 or points is None or points.shape[0] == 0:
            self.num_scans += n if self.observations else 0
            return self
        points, ld, total, offsets, X = self._on_device(points, offsets, X)
        self._reserve(total)
        if self.observations:
            block = (self._mom.data_ptr(), self._mom.numel()) if self.moments else (0, 0)
            with torch.cuda.device(self.device):
                for lo_scan in range(0, n, _lib.VOXEL_OBSERVATIONS_MAX_SCANS):
                    scans = min(n - lo_scan, _lib.VOXEL_OBSERVATIONS_MAX_SCANS)
                    _lib.check(_lib.lib().rdm_voxel_map_integrate_observed(
                        *self._head(), self.voxel, points.data_ptr(), ld, total, offsets.data_ptr() + 8 * lo_scan, X.data_ptr() + 128 * lo_scan,
                        scans, lo, hi, *block, self._obs.data_ptr(), self._obs.numel(), self.num_scans + lo_scan, _lib.stream_ptr()),
                        'rdm_voxel_map_integrate_observed')
            self.num_scans += n
            return self
        name = 'rdm_voxel_map_integrate' + ('_moments' if self.moments else '')
        block = (self._mom.data_ptr(), self._mom.numel()) if self.moments else ()
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), name)(*self._head(), self.voxel, points.data_ptr(), ld, total, offsets.data_ptr(), X.data_ptr(),
                                                 n, lo, hi, *block, _lib.stream_ptr()), name)
        return self

    def extract(self, min_points=1):
        """-> (points float32 [M, C], counts int32 [M], cells int32 [M, 3]) on the device: the voxels with at least min_points
        points in ascending order of (cell x, cell y, cell z); points = the per-voxel means.  Two read-backs (sizes)."""
        points, counts, cells = self._extract('rdm_voxel_map_extract', min_points, ((torch.float32, (self.channels,)), (torch.int32, (1, 3))))
        return points, counts.view(-1), cells

    def _extract(self, name, min_points, blocks, *block_args):
        """The frame of both extracts: reads `occupied`, makes one allocation per (dtype, widths) of `blocks` and cuts it into one
        [occupied, width] output per width, calls `name` (block_args: what it takes between the map and the voxel), reads the number
        of rows it wrote and slices the outputs to it."""
        L = _lib.lib()
        rows = self.stats()['occupied']
        R, dev = max(rows, 1), self.device
        outs = []
        for dtype, widths in blocks:
            flat, lo = torch.empty((R * sum(widths),), dtype=dtype, device=dev), 0
            for w in widths:
                outs.append(flat[lo * R:(lo + w) * R].view(R, w))
                lo += w
        n_rows = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ws = scratch(dev, L.rdm_voxel_map_extract_workspace_bytes(self.capacity))
            _lib.check(getattr(L, name)(*self._head(), *block_args, self.voxel, int(min_points), *(t.data_ptr() for t in outs), rows,
                                        n_rows.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), name)
        m = int(n_rows.item())
        return tuple(t[:m] for t in outs)

    def _need_observations(self, what):
        if not self.observations:
            raise ValueError(f'VoxelMap.{what} needs a map created with observations=True')

    def extract_observations(self, min_points=1):
        """-> (scans, first, last), int32 [M] each on the device, row-aligned with extract(min_points): in how many distinct scans the
        voxel was seen, and the smallest and the largest of their ids.  Two read-backs (sizes)."""
        self._need_observations('extract_observations')
        return tuple(t.view(-1) for t in self._extract('rdm_voxel_map_extract_observations', min_points, ((torch.int32, (1, 1, 1)),),
                                                       self._obs.data_ptr(), self._obs.numel()))

    def pruned(self, min_scans, min_points=1):
        """-> a new VoxelMap of the same capacity and options that holds only the voxels with at least min_points points seen in at
        least min_scans scans (rdm_voxel_map_prune), with their moments and observations where this map has them: `extract`,
        `extract_moments`, `sharpness` and `register` work on it as on any map.  Its `occupied` and `integrated` count what was kept; the
        other counters and num_scans are this map's.  This map is only read.  No read-back."""
        self._need_observations('pruned')
        min_scans, min_points = int(min_scans), int(min_points)
        if min_scans < 0 or min_points < 0:
            raise ValueError(f'min_scans and min_points must be >= 0, got {min_scans} and {min_points}')
        L = _lib.lib()
        out = VoxelMap(self.voxel, self.channels, self.capacity, self.device, self.moments, True)
        old, new = (self._buf.data_ptr(), self._buf.numel(), self.capacity), (out._buf.data_ptr(), out._buf.numel(), out.capacity)
        with torch.cuda.device(self.device):
            _lib.check(L.rdm_voxel_map_prune(*old, self._obs.data_ptr(), self._obs.numel(), *new, self.channels, min_points, min_scans,
                                             _lib.stream_ptr()), 'rdm_voxel_map_prune')
            for attr, kind in self._owned()[1:]:
                self._rehash_beside(kind, old, getattr(self, attr), new, getattr(out, attr))
        out.num_scans, out._bound = self.num_scans, self._bound
        return out

    def _need_moments(self, what):
        if not self.moments:
            raise ValueError(f'VoxelMap.{what} needs a map created with moments=True')

    def extract_moments(self, min_points=1):
        """-> (sums int64 [M, 9], cov float64 [M, 6], eigenvalues float64 [M, 3], normals float64 [M, 3]) on the device, row-aligned
        with extract(min_points).  sums: of u_x, u_y, u_z, u_x u_x, u_x u_y, u_x u_z, u_y u_y, u_y u_z, u_z u_z over the voxel's points,
        u = the 12-bit local coordinate; cov: the population covariance in m^2 (xx, xy, xz, yy, yz, zz); eigenvalues ascending; normals:
        the unit eigenvector of the smallest, its component of largest magnitude positive.  Two read-backs (sizes)."""
        self._need_moments('extract_moments')
        return self._extract('rdm_voxel_map_extract_moments', min_points,
                             ((torch.int64, (_lib.VOXEL_MOMENTS_PLANES,)), (torch.float64, (6, 3, 3))), self._mom.data_ptr(), self._mom.numel())

    def sharpness(self, min_points=4):
        """The ground-truth-free map report over the voxels with at least min_points points (4: the smallest count at which a
        3 x 3 population covariance can have full rank) -> dict: voxels (all occupied), qualified (count >= min_points), degenerate
        (qualified without smallest eigenvalue > 0), plane_thickness = sqrt(mean(max(l0, 0))) in metres over the qualified, entropy =
        the mean of 0.5 ln((2 pi e)^3 l0 l1 l2) over the qualified that are not degenerate (mean plane variance and mean map entropy
        after Razlaw et al. and Droeschel & Behnke).  Lower is sharper for both; nan where there is no voxel to average.  Reduced on
        the device; one read-back beside extract_moments'."""
        import math
        self._need_moments('sharpness')
        if int(min_points) < 1:
            raise ValueError(f'min_points must be >= 1, got {min_points}')
        eig = self.extract_moments(min_points)[2]
        voxels, qualified = self._bound, int(eig.shape[0])  # (extract_moments has just read `occupied`)
        full = eig[:, 0] > 0
        k = (2.0 * math.pi * math.e) ** 3
        product = torch.where(full, k * eig[:, 0] * eig[:, 1] * eig[:, 2], 1.0)  # (ln 1 = 0 for the degenerate: no gather, no read-back)
        out = torch.stack([full.sum().double(), eig[:, 0].clamp_min(0.0).sum(), (0.5 * torch.log(product)).sum()])
        n_full, thick, ent = out.cpu().tolist()
        n_full = int(n_full)
        return dict(voxels=voxels, qualified=qualified, degenerate=qualified - n_full,
                    plane_thickness=math.sqrt(thick / qualified) if qualified else float('nan'),
                    entropy=ent / n_full if n_full else float('nan'))

    def register(self, clouds, poses, *, sigma=0.02, min_points=4, neighbors=1, max_iteration=30, rot_eps=1e-5, trans_eps=1e-4,
                 min_range=0.0, max_range=float('inf'), robust_scale=None):
        """Scan-to-map registration on the per-voxel Gaussians (rdm_voxel_map_register): every scan of the batch
        is registered, from its initial pose, against this map -- point-to-distribution, the NDT / voxelised-GICP family.  clouds,
        poses, min_range, max_range: as `integrate` takes them (poses: the initial poses).  sigma: the isotropic noise of a scan point
        in metres, added to every voxel's covariance; a voxel takes part with at least min_points points; neighbors 1 (the point's own
        voxel) or 7 (and its six face neighbours: a wider basin, less accurate from a small error); at most max_iteration Gauss-Newton
        updates, until one is below rot_eps (rad) and trans_eps (m).  robust_scale mu: None (every pair has weight one) or a positive
        finite number in units of squared Mahalanobis distance: a pair at the distance d2 = r^T M r is weighted by (mu / (mu + d2))^2
        (Geman-McClure, rdm_voxel_map_register_robust), so that an object which stands elsewhere in the scan than in the map does not
        pull the pose; 9 is a value to start from.  The result's weight_sum is then the correspondences by weight.  The map is only
        read.  -> MapRegistrationResult (device tensors).  One 4-byte read-back per eight iterations."""
        self._need_moments('register')
        if robust_scale is not None:
            if isinstance(robust_scale, (str, bytes, bool)) or not isinstance(robust_scale, numbers.Real) or not (
                    0 < float(robust_scale) < float('inf')):
                raise ValueError(f'robust_scale must be None or a positive finite number, got {robust_scale!r}')
            robust_scale = float(robust_scale)
        points, offsets, n, X, lo, hi = self._packed('register', clouds, poses, min_range, max_range)
        sigma, rot_eps, trans_eps = float(sigma), float(rot_eps), float(trans_eps)
        min_points, neighbors, max_iteration = int(min_points), int(neighbors), int(max_iteration)
        self._options(sigma, neighbors, min_points >= 1 and max_iteration >= 0 and rot_eps >= 0 and trans_eps >= 0,
                      'min_points >= 1, max_iteration >= 0, rot_eps >= 0 and trans_eps >= 0')

        def call(outs, weight_sum, tail):
            pts, ld, total, off, Xd = self._on_device(points, offsets, X)
            head = (*self._head(), self._mom.data_ptr(), self._mom.numel(), self.voxel, pts.data_ptr(), ld, total, off.data_ptr(),
                    Xd.data_ptr(), n, lo, hi, sigma, min_points, neighbors, max_iteration, rot_eps, trans_eps)
            if robust_scale is None:
                _lib.check(_lib.lib().rdm_voxel_map_register(*head, *outs, *tail), 'rdm_voxel_map_register')
            else:
                _lib.check(_lib.lib().rdm_voxel_map_register_robust(*head, robust_scale, *outs, weight_sum, *tail),
                           'rdm_voxel_map_register_robust')

        return self._gauss_newton(n, robust_scale is not None, 'rdm_voxel_map_register_workspace_bytes', call)

    def align(self, sources, poses, *, sigma=0.02, min_points=4, source_min_points=4, neighbors=7, max_iteration=30, rot_eps=1e-5,
              trans_eps=1e-4):
        """Map-to-map alignment on the per-voxel Gaussians of both sides (rdm_voxel_map_align): every source is
        aligned, from its initial pose (this map's frame <- the source's), against this map -- distribution-to-distribution, voxelised
        GICP.  sources: a list whose items are each a VoxelMap with moments or a state dict (`state` / `read_state`) that holds
        `moments`, all of one voxel size, which may differ from this map's; a VoxelMap is exported on the device, a state's arrays are
        copied to it.  The same source given twice with two poses is two hypotheses.  poses: [n, 4, 4] finite.  A source voxel takes
        part with at least source_min_points points, a voxel of this map with at least min_points; sigma, neighbors, max_iteration,
        rot_eps and trans_eps as `register` takes them.  The basin is about one voxel of this map with neighbors=7: the start must come
        from elsewhere.  Both maps are only read.  -> MapRegistrationResult (num_points: the source records that passed)."""
        import numpy as np
        self._need_moments('align')
        if not isinstance(sources, (list, tuple)):
            raise ValueError('VoxelMap.align: sources must be a list of VoxelMaps or state dicts')
        packed, source_voxel = [], None
        for i, src in enumerate(sources):
            if isinstance(src, VoxelMap):
                if not src.moments:
                    raise ValueError(f'sources[{i}] needs a map created with moments=True')
                if src.device != self.device:
                    raise ValueError(f'sources[{i}] is on {src.device}, the map on {self.device}')
                voxel, st = src.voxel, src._export(1, moments=True, observations=False)
            elif isinstance(src, dict):
                if src.get('moments') is None:
                    raise ValueError(f'sources[{i}] holds no moments')
                voxel, st = float(src['voxel']), src
            else:
                raise ValueError(f'sources[{i}] must be a VoxelMap or a state dict, got {type(src).__name__}')
            if source_voxel is None:
                source_voxel = voxel
            elif voxel != source_voxel:
                raise ValueError(f'sources[{i}]: voxel differs ({voxel!r} against {source_voxel!r}); one call takes sources of one voxel size')
            rows = int(st['counts'].shape[0])
            arrays = []
            for k, dtype, width in (('counts', torch.uint32, None), ('sums', torch.int64, 3), ('moments', torch.int64, _lib.VOXEL_MOMENTS_PLANES)):
                t = st[k]
                t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
                good = isinstance(t, torch.Tensor) and t.dtype == dtype and t.shape[0] == rows and (
                    t.dim() == 1 if width is None else t.dim() == 2 and (t.shape[1] >= 3 if k == 'sums' else t.shape[1] == width))
                if not good:
                    raise ValueError(f'sources[{i}]: {k} must be {dtype} [{rows}' + ('' if width is None else f', {width}') + '], got '
                                     f'{getattr(t, "dtype", type(t).__name__)} {list(getattr(t, "shape", ()))}')
                arrays.append(t.to(self.device)[:, :3] if k == 'sums' else t.to(self.device))
            packed.append(arrays)
        n = len(packed)
        X = self._poses_arg(poses, n, 'source')
        sigma, rot_eps, trans_eps = float(sigma), float(rot_eps), float(trans_eps)
        min_points, source_min_points, neighbors, max_iteration = int(min_points), int(source_min_points), int(neighbors), int(max_iteration)
        self._options(sigma, neighbors, min_points >= 1 and source_min_points >= 1 and max_iteration >= 0 and rot_eps >= 0 and trans_eps >= 0,
                      'min_points >= 1, source_min_points >= 1, max_iteration >= 0, rot_eps >= 0 and trans_eps >= 0')

        def call(outs, _, tail):
            dev = self.device
            offsets = torch.tensor([0] + [int(a[0].shape[0]) for a in packed], dtype=torch.int64).cumsum(0)
            total = int(offsets[-1])
            if total > 0:
                counts, sums, moments = (torch.cat([a[k] for a in packed]).contiguous() for k in range(3))
            else:  # one placeholder record, never read
                counts = torch.zeros((1,), dtype=torch.uint32, device=dev)
                sums, moments = (torch.zeros((1, w), dtype=torch.int64, device=dev) for w in (3, _lib.VOXEL_MOMENTS_PLANES))
            offsets, Xd = offsets.to(dev), torch.from_numpy(X).to(dev)
            _lib.check(_lib.lib().rdm_voxel_map_align(*self._head(), self._mom.data_ptr(), self._mom.numel(), self.voxel, counts.data_ptr(),
                                                      sums.data_ptr(), 3, moments.data_ptr(), source_voxel, total, offsets.data_ptr(),
                                                      Xd.data_ptr(), n, sigma, min_points, source_min_points, neighbors, max_iteration,
                                                      rot_eps, trans_eps, *outs, *tail), 'rdm_voxel_map_align')

        return self._gauss_newton(n, False, 'rdm_voxel_map_align_workspace_bytes', call)

    def query(self, clouds, poses, *, sigma=0.02, min_points=1, neighbors=1, min_scans=1, max_d2=float('inf'), min_range=0.0,
              max_range=float('inf'), outputs=None):
        """What the map says about every point of every scan (rdm_voxel_map_query).  clouds, poses, min_range,
        max_range: as `integrate` takes them.  A point is gated as `integrate` gates it, looks up its voxel (neighbors = 7: and the six
        face neighbours) under `register`'s rule -- a voxel takes part with at least min_points points -- and is judged by the voxel of
        the smallest Mahalanobis distance d2 = r^T (cov + sigma^2 I)^-1 r (a map without moments: cov = 0): no voxel -> unmapped; that
        voxel seen in fewer than min_scans scans -> transient; d2 > max_d2 -> off_surface; else static.  outputs: an iterable of
        MapQueryResult.FIELDS; None: all that the map supports (`scans`, `first`, `last` need observations).  The others come back as
        None and are not computed.  The map is only read.  -> MapQueryResult (device tensors).  No read-back."""
        points, offsets, n, X, lo, hi = self._packed('query', clouds, poses, min_range, max_range)
        sigma, max_d2 = float(sigma), float(max_d2)
        min_points, neighbors, min_scans = int(min_points), int(neighbors), int(min_scans)
        self._options(sigma, neighbors, min_points >= 1 and min_scans >= 0,
                      f'min_points >= 1 and min_scans >= 0, got {min_points} and {min_scans}')
        if not max_d2 >= 0:
            raise ValueError(f'max_d2 must be >= 0 (inf: no test), got {max_d2}')
        seen = ('scans', 'first', 'last')
        if outputs is None:
            want = set(MapQueryResult.FIELDS) - (set() if self.observations else set(seen))
        else:
            want = set(outputs)
            if want - set(MapQueryResult.FIELDS):
                raise ValueError(f'outputs must be among {MapQueryResult.FIELDS}, got {sorted(want - set(MapQueryResult.FIELDS))}')
        if min_scans > 1 or want & set(seen):
            self._need_observations('query (min_scans > 1, or the outputs scans, first and last)')
        dev = self.device
        rows = 0 if points is None else int(points.shape[0])
        specs = dict(labels=(torch.uint8, ()), best=(torch.int8, ()), counts=(torch.int32, ()), d2=(torch.float64, ()),
                     d2_sum=(torch.float64, ()), pairs=(torch.uint8, ()))
        out = {k: torch.empty((rows,) + shape, dtype=dtype, device=dev) for k, (dtype, shape) in specs.items() if k in want}
        rec = torch.empty((rows, 3), dtype=torch.int32, device=dev) if want & set(seen) else None
        tallies = torch.zeros((n, _lib.VOXEL_QUERY_TALLIES), dtype=torch.int64, device=dev) if 'tallies' in want else None
        if n > 0 and rows > 0:
            points, ld, total, offsets, Xd = self._on_device(points, offsets, X)
            mom = (self._mom.data_ptr(), self._mom.numel()) if self.moments else (0, 0)
            obs = (self._obs.data_ptr(), self._obs.numel()) if self.observations else (0, 0)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().rdm_voxel_map_query(
                    *self._head(), *mom, *obs, self.voxel, points.data_ptr(), ld, total, offsets.data_ptr(), Xd.data_ptr(), n, lo, hi,
                    sigma, min_points, neighbors, min_scans, max_d2, *(_lib.ptr(out.get(k)) for k in ('labels', 'best', 'counts')),
                    _lib.ptr(rec), *(_lib.ptr(out.get(k)) for k in ('d2', 'd2_sum', 'pairs')), _lib.ptr(tallies), _lib.stream_ptr()),
                    'rdm_voxel_map_query')
        else:
            offsets = offsets.to(dev)
        for k, name in enumerate(seen):
            out[name] = rec[:, k] if name in want else None
        return MapQueryResult(tallies=tallies, offsets=offsets, **{k: out.get(k) for k in MapQueryResult.FIELDS if k != 'tallies'})

    def clean(self, clouds, poses, **options):
        """The scans without what the map does not call static: -> (list of tensors, tallies).  clouds: a list of tensors; poses and
        the options: those of `query` (without `outputs`: the labels and the tallies alone are computed).  Tensor i holds the rows of
        clouds[i] with the label `static`, all of its columns, in order; tallies int64 [n, 8] as MapQueryResult's.  One read-back
        (the sizes of the result) per cloud."""
        if not isinstance(clouds, (list, tuple)) or (len(clouds) == 2 and isinstance(clouds[1], torch.Tensor) and clouds[1].dtype == torch.int64):
            raise ValueError('VoxelMap.clean: clouds must be a list of tensors')
        if 'outputs' in options:
            raise ValueError('VoxelMap.clean computes the labels and the tallies: it takes no `outputs`')
        res = self.query(list(clouds), poses, outputs=('labels', 'tallies'), **options)
        keep = res.labels == MapQueryResult.LABELS.index('static')
        edges = [0]
        for t in clouds:
            edges.append(edges[-1] + int(t.shape[0]))
        return [t[keep[a:b]] for t, a, b in zip(clouds, edges, edges[1:])], res.tallies

    # ---- the state: save, load, merge (rdm_voxel_map_export / rdm_voxel_map_import; DESIGN.md section 7, "voxel map state") ----

    def state(self, min_points=1):
        """The raw state of the voxels with at least min_points points, row-aligned with extract(min_points) (rdm_voxel_map_export) ->
        dict: device tensors keys uint64 [M] (ascending), counts uint32 [M], sums int64 [M, C] and, where the map has the blocks,
        moments int64 [M, 9] and observations int32 [M, 3] = {scans, first, last}; host values voxel, channels, num_scans and counters
        (what `stats` returns).  These integers are all a map is: `from_state` rebuilds it from them at any capacity, bit for bit.
        Two read-backs (sizes)."""
        return self._export(min_points)

    def _export(self, min_points, moments=True, observations=True):
        """`state`, without a block that the caller leaves out."""
        L, dev = _lib.lib(), self.device
        counters = self.stats()
        rows = counters['occupied']
        R = max(rows, 1)
        out = dict(keys=torch.empty((R,), dtype=torch.uint64, device=dev), counts=torch.empty((R,), dtype=torch.uint32, device=dev),
                   sums=torch.empty((R, self.channels), dtype=torch.int64, device=dev))
        if self.moments and moments:
            out['moments'] = torch.empty((R, _lib.VOXEL_MOMENTS_PLANES), dtype=torch.int64, device=dev)
        if self.observations and observations:
            out['observations'] = torch.empty((R, 3), dtype=torch.int32, device=dev)
        n_rows = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ws = scratch(dev, L.rdm_voxel_map_extract_workspace_bytes(self.capacity))
            _lib.check(L.rdm_voxel_map_export(*self._head(), *self._blocks(moments, observations), int(min_points), out['keys'].data_ptr(),
                                              out['counts'].data_ptr(), out['sums'].data_ptr(), _lib.ptr(out.get('moments')),
                                              _lib.ptr(out.get('observations')), rows, n_rows.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr()), 'rdm_voxel_map_export')
        m = int(n_rows.item())
        out = {k: t[:m] for k, t in out.items()}
        out.update(voxel=self.voxel, channels=self.channels, num_scans=self.num_scans, counters=counters)
        return out

    def _blocks(self, moments=True, observations=True):
        """(moments, moments_bytes, observations, observations_bytes) as the state calls take them: zeros for a block that the map
        lacks or that the caller leaves out."""
        mom = (self._mom.data_ptr(), self._mom.numel()) if self.moments and moments else (0, 0)
        obs = (self._obs.data_ptr(), self._obs.numel()) if self.observations and observations else (0, 0)
        return mom + obs

    def _import(self, what, state, id_offset, skipped):
        """Adds the records of `state` (device tensors of this map's device) through rdm_voxel_map_import; raises if one was rejected.
        The caller has reserved the room.  One read-back (the rejected records)."""
        rows = int(state['keys'].shape[0])
        host = (ctypes.c_uint64 * 4)(*(int(v) for v in skipped))
        n_rejected = torch.zeros((1,), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rdm_voxel_map_import(
                *self._head(), *self._blocks(), state['keys'].data_ptr(), state['counts'].data_ptr(), state['sums'].data_ptr(),
                state['moments'].data_ptr() if self.moments else 0, state['observations'].data_ptr() if self.observations else 0, rows,
                int(id_offset), ctypes.addressof(host), n_rejected.data_ptr(), _lib.stream_ptr()), 'rdm_voxel_map_import')
        bad = int(n_rejected.item())
        if bad:
            raise ValueError(f'VoxelMap.{what}: {bad} of {rows} records are not records of a voxel map (a key with bit 63 set, a count '
                             'of 0, or observations that no set of scans gives)')

    @classmethod
    def from_state(cls, state, device='cuda', capacity=None, moments=None, observations=None):
        """A map from what `state` or `read_state` returned (device tensors, host tensors or numpy arrays).  moments / observations
        None: as the state has them; True for a block that the state lacks is a ValueError; False drops the block.  capacity None:
        the smallest power of two >= max(64, 2 rows).  `extract`, `extract_moments`, `extract_observations`, `stats`, `num_scans`,
        `register` and `query` of the result are, bit for bit, those of the map the state was taken from (with min_points = 1)."""
        import numpy as np
        have = {k: state.get(k) is not None for k in ('moments', 'observations')}
        want = {}
        for k, asked in (('moments', moments), ('observations', observations)):
            if asked and not have[k]:
                raise ValueError(f'VoxelMap.from_state: {k}=True, but the state holds no {k}')
            want[k] = have[k] if asked is None else bool(asked)
        channels = int(state['channels'])
        rows = int(state['keys'].shape[0])
        shapes = dict(keys=(torch.uint64, (rows,)), counts=(torch.uint32, (rows,)), sums=(torch.int64, (rows, channels)),
                      moments=(torch.int64, (rows, _lib.VOXEL_MOMENTS_PLANES)), observations=(torch.int32, (rows, 3)))
        if capacity is None:
            capacity = 64
            while capacity < 2 * rows:
                capacity *= 2
        out = cls(float(state['voxel']), channels, int(capacity), device, want['moments'], want['observations'])
        dev_state = {}
        for k, (dtype, shape) in shapes.items():
            if k in want and not want[k]:
                continue
            t = state[k]
            t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError(f'VoxelMap.from_state: {k} must be {dtype} {list(shape)}, got '
                                 f'{getattr(t, "dtype", type(t).__name__)} {list(getattr(t, "shape", ()))}')
            dev_state[k] = t.to(out.device).contiguous()
        counters = state['counters']
        if not isinstance(counters, dict):
            counters = dict(zip(_lib.VOXEL_MAP_STATS, (int(v) for v in counters)))
        out._reserve(rows)
        out._import('from_state', dev_state, 0, [counters[k] for k in _lib.VOXEL_MAP_STATS[2:]])
        out.num_scans = int(state['num_scans'])
        return out

    def save(self, path):
        """The whole map into one .npz (`write_state`): `VoxelMap.load` gives it back bit for bit.  -> path."""
        write_state(path, self.state())
        return path

    @classmethod
    def load(cls, path, device='cuda', capacity=None, moments=None, observations=None):
        """The map that `save` wrote to `path`: from_state(read_state(path), ...)."""
        return cls.from_state(read_state(path), device, capacity, moments, observations)

    def merge(self, other, id_offset=None):
        """Adds the map `other` of OTHER scans into this one: afterwards this map is, bit for bit, the map of the scans of both --
        every sum, all six counters, and with observations the scans of `other` numbered on from id_offset (None: num_scans; then
        num_scans = max(num_scans, id_offset + other.num_scans)).  Both maps need the same voxel, channels and device, and `other` the
        blocks that this map keeps (a block that only `other` has is left out).  `other` is exported on the device and imported
        here (rdm_voxel_map_export / rdm_voxel_map_import): one record path.  `other` is only read.  -> self."""
        if not isinstance(other, VoxelMap):
            raise ValueError('VoxelMap.merge: other must be a VoxelMap')
        if other.voxel != self.voxel:
            raise ValueError(f'VoxelMap.merge: voxel differs ({other.voxel!r} against {self.voxel!r}); maps add only on the same grid')
        if other.channels != self.channels:
            raise ValueError(f'VoxelMap.merge: channels differ ({other.channels} against {self.channels})')
        if other.device != self.device:
            raise ValueError(f'VoxelMap.merge: device differs ({other.device} against {self.device})')
        for k in ('moments', 'observations'):
            if getattr(self, k) and not getattr(other, k):
                raise ValueError(f'VoxelMap.merge: other has no {k}, which this map keeps')
        id_offset = self.num_scans if id_offset is None else int(id_offset)
        if id_offset < 0:
            raise ValueError(f'VoxelMap.merge: id_offset must be >= 0, got {id_offset}')
        if id_offset + other.num_scans > 2 ** 31 - 1:
            raise ValueError(f'VoxelMap.merge: ids overflow ({id_offset} + {other.num_scans} scans; ids lie in [0, 2^31 - 1))')
        st = other._export(1, self.moments, self.observations)
        rows, counters = int(st['keys'].shape[0]), st['counters']
        self._reserve(rows)
        self._import('merge', st, id_offset, [counters[k] for k in _lib.VOXEL_MAP_STATS[2:]])
        self.num_scans = max(self.num_scans, id_offset + other.num_scans)
        return self


_STATE_FORMAT, _STATE_VERSION = 'rdmnet_amd.voxel_map', 1
_STATE_ARRAYS = dict(keys=('uint64', ()), counts=('uint32', ()), sums=('int64', (None,)), moments=('int64', (_lib.VOXEL_MOMENTS_PLANES,)),
                     observations=('int32', (3,)))


def write_state(path, state):
    """What VoxelMap.state returned (tensors or numpy arrays) into the one .npz file `path`: format = 'rdmnet_amd.voxel_map', version
    = 1, voxel (float64), channels, frac_bits, moments_shift, num_scans, counters (uint64 [6], VOXEL_MAP_STATS' order) and the
    arrays keys, counts, sums and, where the state has them, moments and observations.  No GPU is needed."""
    import numpy as np
    counters = state['counters']
    if isinstance(counters, dict):
        counters = [counters[k] for k in _lib.VOXEL_MAP_STATS]
    arrays = {}
    for k, (dtype, _) in _STATE_ARRAYS.items():
        t = state.get(k)
        if t is not None:
            arrays[k] = np.ascontiguousarray((t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype, copy=False))
    with open(path, 'wb') as f:
        np.savez(f, format=np.array(_STATE_FORMAT), version=np.int64(_STATE_VERSION), voxel=np.float64(state['voxel']),
                 channels=np.int64(state['channels']), frac_bits=np.int64(_lib.VOXEL_MAP_FRAC_BITS),
                 moments_shift=np.int64(_lib.VOXEL_MOMENTS_SHIFT), num_scans=np.int64(state['num_scans']),
                 counters=np.asarray(counters, np.uint64), **arrays)


def read_state(path):
    """The state that write_state wrote to `path` -> dict of numpy arrays and host values as VoxelMap.state's (counters: a dict), read
    with allow_pickle=False and checked: a file that is not such a state, or whose records no map can hold, is a ValueError that says
    what is wrong.  No GPU is needed."""
    import numpy as np

    def bad(why):
        return ValueError(f'{path}: {why}')

    with np.load(path, allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    for k in ('format', 'version', 'voxel', 'channels', 'frac_bits', 'moments_shift', 'num_scans', 'counters', 'keys', 'counts', 'sums'):
        if k not in data:
            raise bad(f"not a voxel map state: no '{k}'")
    if data['format'].shape != () or str(data['format']) != _STATE_FORMAT:
        raise bad(f"not a voxel map state: format {str(data['format'])!r}, expected {_STATE_FORMAT!r}")
    if int(data['version']) != _STATE_VERSION:
        raise bad(f"version {int(data['version'])}, this library reads version {_STATE_VERSION}")
    if int(data['frac_bits']) != _lib.VOXEL_MAP_FRAC_BITS:
        raise bad(f"frac_bits {int(data['frac_bits'])}, the library has {_lib.VOXEL_MAP_FRAC_BITS}")
    if int(data['moments_shift']) != _lib.VOXEL_MOMENTS_SHIFT:
        raise bad(f"moments_shift {int(data['moments_shift'])}, the library has {_lib.VOXEL_MOMENTS_SHIFT}")
    voxel, channels, num_scans = float(data['voxel']), int(data['channels']), int(data['num_scans'])
    if not (voxel > 0 and voxel < float('inf')) or not 3 <= channels <= _lib.VOXEL_MAP_MAX_CHANNELS or not 0 <= num_scans <= 2 ** 31 - 1:
        raise bad(f'voxel {voxel}, channels {channels}, num_scans {num_scans}: not those of a voxel map')
    if data['counters'].dtype != np.uint64 or data['counters'].shape != (len(_lib.VOXEL_MAP_STATS),):
        raise bad(f"counters must be uint64 [{len(_lib.VOXEL_MAP_STATS)}], got {data['counters'].dtype} {list(data['counters'].shape)}")
    rows = data['keys'].shape[0] if data['keys'].ndim == 1 else -1
    out = {}
    for k, (dtype, tail) in _STATE_ARRAYS.items():
        if k not in data:
            continue
        shape = (rows,) + tuple(channels if w is None else w for w in tail)
        if data[k].dtype != np.dtype(dtype) or data[k].shape != shape:
            raise bad(f'{k} must be {dtype} {list(shape) if rows >= 0 else "[M]"}, got {data[k].dtype} {list(data[k].shape)}')
        out[k] = data[k]
    keys = out['keys']
    if (keys >> np.uint64(63)).any() or not (keys[1:] > keys[:-1]).all():
        raise bad('keys must ascend strictly with bit 63 clear')
    if not (out['counts'] >= 1).all():
        raise bad('counts must be >= 1')
    if 'moments' in out and not (out['moments'] >= 0).all():
        raise bad('moments must be >= 0 (sums of non-negative local coordinates)')
    if 'observations' in out:
        scans, first, last = (out['observations'][:, k].astype(np.int64) for k in range(3))
        if not ((1 <= scans) & (scans <= last - first + 1) & (0 <= first) & (first <= last) & (last <= 2 ** 31 - 2)).all():
            raise bad('observations must hold 1 <= scans <= last - first + 1 and 0 <= first <= last <= 2^31 - 2')
    out.update(voxel=voxel, channels=channels, num_scans=num_scans,
               counters=dict(zip(_lib.VOXEL_MAP_STATS, (int(v) for v in data['counters']))))
    return out


class MapRegistrationResult:
    """What VoxelMap.register returns, device tensors with one row per scan: transformations float64 [n, 4, 4] (the refined poses),
    information float64 [n, 6, 6] (H = the sum of J^T M J at the returned pose, rotation first: usable as the weight of a scan-to-map
    edge), gradient float64 [n, 6], cost float64 [n] (the sum of r^T M r), and int64 [n] each: iterations (updates applied),
    num_correspondences (point-voxel pairs of the last evaluation), num_points (rows that passed the gates) and status (STATUS).
    weight_sum: None, or with register's robust_scale float64 [n], the sum of the pairs' weights (num_correspondences by weight);
    information, gradient and cost are then the weighted sums."""
    STATUS = ('max_iteration', 'converged', 'degenerate')

    def __init__(self, transformations, information, gradient, cost, iterations, num_correspondences, num_points, status, weight_sum=None):
        self.transformations, self.information, self.gradient, self.cost = transformations, information, gradient, cost
        self.iterations, self.num_correspondences, self.num_points, self.status = iterations, num_correspondences, num_points, status
        self.weight_sum = weight_sum

    def __repr__(self):
        rows = torch.stack([self.iterations, self.num_correspondences, self.num_points, self.status]).cpu().tolist()
        cost = self.cost.cpu().tolist()
        by_weight = [''] * len(cost) if self.weight_sum is None else [f' ({w:.6g} by weight)' for w in self.weight_sum.cpu().tolist()]
        return 'MapRegistrationResult(' + '; '.join(
            f'{k}: {self.STATUS[s] if 0 <= s < 3 else s} after {i} updates, {c} correspondences{w} of {p} points, cost {v:.6g}'
            for k, (i, c, p, s, v, w) in enumerate(zip(*rows, cost, by_weight))) + ')'


class MapQueryResult:
    """What VoxelMap.query returns: device tensors indexed by the row of the packed batch (scan i is rows offsets[i] .. offsets[i + 1]),
    None where not asked for.  labels uint8 (codes into LABELS); best int8 (which of the visited voxels won: 0 the point's own, 1 ... 6
    its -x, +x, -y, +y, -z, +z neighbour, -1 none); counts int32 (that voxel's points, or 0); scans, first, last int32 (its
    observations, or 0, 2^31 - 1, -1); d2 float64 (its Mahalanobis distance, or inf); d2_sum float64 (over all voxels that took part:
    `register`'s cost term of the row); pairs uint8 (how many took part); tallies int64 [n, 8] (per scan the rows of each label, then
    the sum of pairs); offsets int64 [n + 1]."""
    LABELS = _lib.VOXEL_POINT_LABELS
    FIELDS = ('labels', 'best', 'counts', 'scans', 'first', 'last', 'd2', 'd2_sum', 'pairs', 'tallies')

    def __init__(self, labels, best, counts, scans, first, last, d2, d2_sum, pairs, tallies, offsets):
        self.labels, self.best, self.counts, self.scans, self.first, self.last = labels, best, counts, scans, first, last
        self.d2, self.d2_sum, self.pairs, self.tallies, self.offsets = d2, d2_sum, pairs, tallies, offsets

    def __repr__(self):
        if self.tallies is None:
            return f'MapQueryResult({int(self.offsets.numel()) - 1} scans)'
        return 'MapQueryResult(' + '; '.join(
            f'{k}: ' + ', '.join(f'{v} {name}' for name, v in zip(self.LABELS, row) if v) for k, row in enumerate(self.tallies.cpu().tolist())) + ')'


class RegistrationResult:
    """Named as Open3D's: transformation (float64 [4, 4], numpy), fitness, inlier_rmse, num_correspondences (of the last
    evaluation), iterations (updates applied) and, when asked for, history (float64 [evaluations, 15] numpy: per
    evaluation k {fitness, rmse, n_corr, update_k as 12 row-major R|t values}; row 0 is the initial evaluation)."""

    def __init__(self, transformation, fitness, inlier_rmse, num_correspondences, iterations, history=None,
                 correspondence_set=None):
        self.transformation = transformation
        self.correspondence_set = correspondence_set  # evaluate_registration: int64 CUDA [C, 2], rows (source row, target row)
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.num_correspondences = num_correspondences
        self.iterations = iterations
        self.history = history

    def __repr__(self):
        return (f'RegistrationResult(fitness={self.fitness:.6e}, inlier_rmse={self.inlier_rmse:.6e}, '
                f'num_correspondences={self.num_correspondences}, iterations={self.iterations})')


def _points_arg(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= 3):
        raise ValueError(f'{name} must be a float32 CUDA tensor [N, >=3]')
    if t.shape[0] > 0 and t.stride(1) != 1:
        raise ValueError(f'{name} must have unit column stride')
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def icp_point_to_point(source, target, max_correspondence_distance, init=None, max_iteration=30, relative_fitness=1e-6,
                       relative_rmse=1e-6, history=False):
    """Open3D's registration_icp with TransformationEstimationPointToPoint (no scaling) and ICPConvergenceCriteria (the
    defaults are Open3D's), as preporcess/generate_kitti_pairs.py:157-172 runs it, on the GPU (rdm_icp_point_to_point).
    source / target: float32 CUDA [N, >=3] (xyz first).  init: 4x4 (anything numpy accepts), None = identity.
    -> RegistrationResult with host values (the call ends with the read-back of its results)."""
    import numpy as np
    L = _lib.lib()
    lds, ldt = _points_arg(source, 'source'), _points_arg(target, 'target')
    if source.device != target.device:
        raise ValueError('source and target must be on the same device')
    if not max_correspondence_distance > 0:
        raise ValueError(f'max_correspondence_distance must be > 0, got {max_correspondence_distance}')
    if int(max_iteration) < 0:
        raise ValueError(f'max_iteration must be >= 0, got {max_iteration}')
    init64 = np.eye(4) if init is None else np.ascontiguousarray(np.asarray(init, dtype=np.float64))
    if init64.shape != (4, 4):
        raise ValueError(f'init must be 4x4, got {init64.shape}')
    dev = source.device
    out = torch.empty((20,), dtype=torch.float64, device=dev)  # transform[16], fitness, rmse, stats (2 x int32) in one read-back
    stats = out[18:].view(torch.int32)
    hist = torch.empty((int(max_iteration) + 1, 15), dtype=torch.float64, device=dev) if history else None
    ws = scratch(dev, L.rdm_icp_workspace_bytes(source.shape[0], target.shape[0]))
    _lib.check(L.rdm_icp_point_to_point(_lib.ptr(source), source.shape[0], lds, _lib.ptr(target), target.shape[0], ldt,
                                        float(max_correspondence_distance), init64.ctypes.data, int(max_iteration),
                                        float(relative_fitness), float(relative_rmse), out.data_ptr(), out[16:].data_ptr(),
                                        stats.data_ptr(), _lib.ptr(hist), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_icp_point_to_point')
    host = out.cpu().numpy()
    iters, n_corr = (int(x) for x in host[18:19].view(np.int32))
    h = hist[:iters + 1].cpu().numpy() if history else None
    return RegistrationResult(host[:16].reshape(4, 4).copy(), float(host[16]), float(host[17]), n_corr, iters, h)


def icp_correspondences(pcd, target, max_correspondence_distance):
    """The evaluation step of icp_point_to_point alone: pcd float64 CUDA [N, 3] (contiguous), target float32 CUDA
    [M, >=3] -> (idx int32 [N], -1 = none; d2 float64 [N], -1 where idx is -1), on the device."""
    L = _lib.lib()
    if not (isinstance(pcd, torch.Tensor) and pcd.is_cuda and pcd.dtype == torch.float64 and pcd.dim() == 2 and pcd.shape[1] == 3):
        raise ValueError('pcd must be a float64 CUDA tensor [N, 3]')
    pcd = pcd.contiguous()
    ldt = _points_arg(target, 'target')
    if not max_correspondence_distance > 0:
        raise ValueError(f'max_correspondence_distance must be > 0, got {max_correspondence_distance}')
    n = pcd.shape[0]
    idx = torch.empty((max(n, 1),), dtype=torch.int32, device=pcd.device)
    d2 = torch.empty((max(n, 1),), dtype=torch.float64, device=pcd.device)
    ws = scratch(pcd.device, L.rdm_icp_workspace_bytes(0, target.shape[0]))
    _lib.check(L.rdm_icp_correspondences(_lib.ptr(pcd), n, _lib.ptr(target), target.shape[0], ldt,
                                         float(max_correspondence_distance), idx.data_ptr(), d2.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _lib.stream_ptr()),
               'rdm_icp_correspondences')
    return idx[:n], d2[:n]


def _transform_arg(transform, name):
    """None, or anything numpy / torch holds as a 4x4 -> a contiguous float64 host array (kept alive by the caller)."""
    import numpy as np
    if transform is None:
        return None
    if isinstance(transform, torch.Tensor):
        transform = transform.detach().cpu().numpy()
    T = np.ascontiguousarray(np.asarray(transform, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError(f'{name}: transform must be 4x4, got {T.shape}')
    return T


def _ball_count(ref_points, src_points, transform, radius, name, want_min=False, want_hits=False):
    """rdm_ball_count -> (totals (C, ref rows, src rows, status), ws, ref_min_d2, ref_hit, src_hit); the workspace holds the index,
    counts and offsets rdm_ball_fill reads."""
    if radius is None or not radius > 0:
        raise ValueError(f'{name} must be > 0, got {radius}')
    L = _lib.lib()
    ldr, lds = _points_arg(ref_points, 'ref_points'), _points_arg(src_points, 'src_points')
    if ref_points.device != src_points.device:
        raise ValueError('ref_points and src_points must be on the same device')
    T = _transform_arg(transform, name)
    dev = ref_points.device
    n, m = ref_points.shape[0], src_points.shape[0]
    ref_min = torch.empty((max(n, 1),), dtype=torch.float64, device=dev) if want_min else None
    ref_hit = torch.empty((max(n, 1),), dtype=torch.uint8, device=dev) if want_hits else None
    src_hit = torch.empty((pad4(max(m, 1)),), dtype=torch.uint8, device=dev) if want_hits else None
    # (a buffer of its own, not the shared scratch: the fill call reads it after other ops may have run)
    ws = torch.empty((L.rdm_ball_workspace_bytes(n, m),), dtype=torch.uint8, device=dev)
    totals = (ctypes.c_int64 * 4)()
    _lib.check(L.rdm_ball_count(_lib.ptr(ref_points), n, ldr, _lib.ptr(src_points), m, lds, 0 if T is None else T.ctypes.data,
                                float(radius), _lib.ptr(ref_min), _lib.ptr(ref_hit), _lib.ptr(src_hit), totals, ws.data_ptr(),
                                ws.numel(), _lib.stream_ptr()),
               'rdm_ball_count')
    return tuple(int(x) for x in totals), ws, ref_min, ref_hit, src_hit


def get_correspondences(ref_points, src_points, transform=None, matching_radius=None):
    """get_correspondences (geotransformer/utils/registration.py:203-216) on the GPU (rdm_ball_count + rdm_ball_fill): ref_points /
    src_points float32 CUDA [N, >=3] (xyz first, any row stride), transform 4x4 src -> ref (None: src as it is), read as float64
    -> int64 CUDA [C, 2], every (i, j) with |ref_i - T src_j| <= matching_radius (closed, as cKDTree's ball) in ascending (i, j).
    The only read-back is C."""
    L = _lib.lib()
    totals, ws, _, _, _ = _ball_count(ref_points, src_points, transform, matching_radius, 'matching_radius')
    c = totals[0]
    out = torch.empty((c, 2), dtype=torch.int64, device=ref_points.device)
    if c > 0:
        _lib.check(L.rdm_ball_fill(_lib.ptr(ref_points), ref_points.shape[0], _points_arg(ref_points, 'ref_points'),
                                   src_points.shape[0], out.data_ptr(), c, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
                   'rdm_ball_fill')
    return out


def compute_overlap(ref_points, src_points, transform=None, positive_radius=0.1, both=False):
    """compute_overlap (geotransformer/utils/registration.py:191-197) on the GPU: the fraction of ref rows whose nearest (moved)
    src row is closer than positive_radius (strict) -> float; both=True -> (ref side, src side), the src side being the fraction
    of src rows whose nearest ref row is that close, from the same call.  An empty cloud gives 0.0."""
    o_ref, o_src, _ = pair_overlap(ref_points, src_points, transform, positive_radius, 'positive_radius')
    return (o_ref, o_src) if both else o_ref


def pair_overlap(ref_points, src_points, transform, radius, name='radius'):
    """One count pass (rdm_ball_count, no list) -> (compute_overlap of the ref side, of the src side, the number of
    get_correspondences rows) at `radius`."""
    totals, _, _, _, _ = _ball_count(ref_points, src_points, transform, radius, name)
    n, m = ref_points.shape[0], src_points.shape[0]
    return (totals[1] / n if n > 0 else 0.0), (totals[2] / m if m > 0 else 0.0), totals[0]


def overlap_labels(ref_points, src_points, transform, radius):
    """The per-point labels of loss.py:94-103,155-158 without the list: (ref_gt bool CUDA [N], src_gt bool CUDA [M]), a row being
    true iff it appears in some correspondence of get_correspondences(ref_points, src_points, transform, radius)."""
    _, _, _, ref_hit, src_hit = _ball_count(ref_points, src_points, transform, radius, 'radius', want_hits=True)
    return ref_hit[:ref_points.shape[0]].bool(), src_hit[:src_points.shape[0]].bool()


def _nearest(q_points, s_points, q_transform=None, s_transform=None, cell=None, radius=0.0, want_rows=True):
    """rdm_nearest -> (idx int32 [n_q], d2 float64 [n_q] (None without want_rows), totals (sum of distances, rows nearer than
    radius, their sum of d2, rows that took the exact sweep))."""
    L = _lib.lib()
    ldq, lds = _points_arg(q_points, 'q_points'), _points_arg(s_points, 's_points')
    if q_points.device != s_points.device:
        raise ValueError('q_points and s_points must be on the same device')
    Tq, Ts = _transform_arg(q_transform, 'q_transform'), _transform_arg(s_transform, 's_transform')
    dev = q_points.device
    n, m = q_points.shape[0], s_points.shape[0]
    idx = torch.empty((max(n, 1),), dtype=torch.int32, device=dev) if want_rows else None
    d2 = torch.empty((max(n, 1),), dtype=torch.float64, device=dev) if want_rows else None
    ws = scratch(dev, L.rdm_nearest_workspace_bytes(n, m))
    totals = (ctypes.c_double * 5)()
    _lib.check(L.rdm_nearest(_lib.ptr(q_points), n, ldq, _lib.ptr(s_points), m, lds, 0 if Tq is None else Tq.ctypes.data,
                             0 if Ts is None else Ts.ctypes.data, 0.0 if cell is None else float(cell), float(radius),
                             _lib.ptr(idx), _lib.ptr(d2), totals, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_nearest')
    if want_rows:
        idx, d2 = idx[:n], d2[:n]
    return idx, d2, (float(totals[0]), int(totals[1]), float(totals[2]), int(totals[3]))


def get_nearest_neighbor(q_points, s_points, return_index=False, *, q_transform=None, s_transform=None, cell=None):
    """get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22, a cKDTree k = 1 query) on the GPU (rdm_nearest): q_points /
    s_points float32 CUDA [N, >=3] (xyz first, any row stride), read as float64; q_transform / s_transform: optional 4x4 applied
    to the respective cloud -> float64 CUDA [n_q], the distance of every query row to its nearest support row, at any distance
    (with return_index also int64 [n_q], the LOWEST support row at that distance; n_s = 0: inf and n_s).  cell: the edge of the
    index's cells (None: chosen on the device); the result does not depend on it."""
    idx, d2, _ = _nearest(q_points, s_points, q_transform, s_transform, cell)
    dist = torch.sqrt(d2)
    return (dist, idx.long()) if return_index else dist


def _mean(total, n):
    return total / n if n > 0 else float('nan')  # (numpy's mean of nothing)


def compute_modified_chamfer_distance(raw_points, ref_points, src_points, gt_transform, est_transform):
    """compute_modified_chamfer_distance (geotransformer/utils/registration.py:155-172, RPMNet's measure) on the GPU: the mean
    nearest distance of est . src to raw, plus that of ref to (est . gt^-1) . raw -> float.  The composed transform is formed in
    float64 on the host, as the reference forms it."""
    import numpy as np
    gt, est = _transform_arg(gt_transform, 'gt_transform'), _transform_arg(est_transform, 'est_transform')
    composed = np.matmul(est, np.linalg.inv(gt))
    _, _, p_q = _nearest(src_points, raw_points, q_transform=est, want_rows=False)
    _, _, q_p = _nearest(ref_points, raw_points, s_transform=composed, want_rows=False)
    return _mean(p_q[0], src_points.shape[0]) + _mean(q_p[0], ref_points.shape[0])


def compute_registration_rmse(src_points, gt_transform, est_transform):
    """compute_registration_rmse (geotransformer/utils/registration.py:136-152; the re-alignment error of Rotated 3DMatch) on the
    GPU (rdm_realign_error): the mean over src_points of |gt p - est p| in float64 -> float."""
    L = _lib.lib()
    ld = _points_arg(src_points, 'src_points')
    gt, est = _transform_arg(gt_transform, 'gt_transform'), _transform_arg(est_transform, 'est_transform')
    if gt is None or est is None:
        raise ValueError('compute_registration_rmse: gt_transform and est_transform must be 4x4')
    ws = scratch(src_points.device, L.rdm_nearest_workspace_bytes(0, 0))
    mean = ctypes.c_double()
    _lib.check(L.rdm_realign_error(_lib.ptr(src_points), src_points.shape[0], ld, gt.ctypes.data, est.ctypes.data,
                                   ctypes.byref(mean), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_realign_error')
    return float(mean.value)


def quality_dict(v):
    """The eight numbers of rdm_engine_alignment_quality ({rows nearer than radius, their sum of d2, the sum of all nearest
    distances} of the ref side and of the src side, n_ref, n_src) -> alignment_quality's dict."""
    import math
    n_ref, n_src = int(v[6]), int(v[7])
    out = {}
    for k, (side, n) in enumerate((('ref', n_ref), ('src', n_src))):
        within, sum_d2 = v[3 * k], v[3 * k + 1]
        out[f'fitness_{side}'] = within / n if n > 0 else 0.0
        out[f'inlier_rmse_{side}'] = math.sqrt(sum_d2 / within) if within > 0 else 0.0
    out['chamfer'] = _mean(v[2], n_ref) + _mean(v[5], n_src)
    out['n_ref'], out['n_src'] = n_ref, n_src
    return out


QUALITY_KEYS = ('fitness_ref', 'fitness_src', 'inlier_rmse_ref', 'inlier_rmse_src', 'chamfer')


def alignment_quality(ref_points, src_points, transform, radius):
    """How well `transform` (4x4, src -> ref; None: identity) aligns two clouds, without ground truth: what Open3D's
    evaluate_registration reports, for both sides, plus the chamfer distance.  Both sides are measured in the ref frame (two
    rdm_nearest calls) -> dict(fitness_ref / fitness_src: the share of rows with a neighbour nearer than radius (strict) in the
    other cloud; inlier_rmse_ref / inlier_rmse_src: sqrt of the mean d2 over those rows, 0 without any; chamfer: the sum of the
    two mean nearest distances; n_ref, n_src)."""
    if radius is None or not radius > 0:
        raise ValueError(f'alignment_quality: radius must be > 0, got {radius}')
    _, _, a = _nearest(ref_points, src_points, s_transform=transform, radius=radius, want_rows=False)
    _, _, b = _nearest(src_points, ref_points, q_transform=transform, radius=radius, want_rows=False)
    return quality_dict((float(a[1]), a[2], a[0], float(b[1]), b[2], b[0], ref_points.shape[0], src_points.shape[0]))


INFORMATION_WIDTH = 40  # the read-back of rdm_information_matrix: the matrix [36], C, the sum of d2, rows swept, status


def information_result(host, corr):
    """The read-back of rdm_information_matrix / rdm_engine_information_matrix (40 doubles) and the correspondence buffer ->
    (information float64 [6, 6] (host tensor), C, the sum of d2 over the correspondences, rows that took the sweep, corr[:C])."""
    info = torch.tensor([float(x) for x in host[:36]], dtype=torch.float64).reshape(6, 6)
    c = int(host[36])
    return info, c, float(host[37]), int(host[38]), None if corr is None else corr[:c]


def _information(source, target, radius, s_transform=None, t_transform=None, want_corr=False, cell=None):
    """rdm_information_matrix -> information_result's tuple; s_transform / t_transform move the source / the target cloud."""
    if radius is None or not radius > 0:
        raise ValueError(f'max_correspondence_distance must be > 0, got {radius}')
    L = _lib.lib()
    ldq, lds = _points_arg(source, 'source'), _points_arg(target, 'target')
    if source.device != target.device:
        raise ValueError('source and target must be on the same device')
    Tq, Ts = _transform_arg(s_transform, 'transformation'), _transform_arg(t_transform, 'target transformation')
    dev = source.device
    n, m = source.shape[0], target.shape[0]
    corr = torch.empty((max(n, 1), 2), dtype=torch.int64, device=dev) if want_corr else None  # (at most one row per source row)
    ws = scratch(dev, L.rdm_information_workspace_bytes(n, m))
    host = (ctypes.c_double * INFORMATION_WIDTH)()
    _lib.check(L.rdm_information_matrix(_lib.ptr(source), n, ldq, _lib.ptr(target), m, lds, 0 if Tq is None else Tq.ctypes.data,
                                        0 if Ts is None else Ts.ctypes.data, 0.0 if cell is None else float(cell), float(radius),
                                        host, _lib.ptr(corr), n, ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_information_matrix')
    return information_result(host, corr)


def information_matrix(source, target, max_correspondence_distance, transformation=None, return_correspondences=False):
    """Open3D's get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation) on the GPU
    (rdm_information_matrix; parity unpinned, pinned to tests/information_restatement.py): source / target float32 CUDA [N, >=3]
    (xyz first, any row stride), transformation 4x4 source -> target (None: the source as it is), read as float64.  A source row
    has a correspondence iff its nearest target row (the lowest among equal distances) is nearer than
    max_correspondence_distance (strict); the matrix sums g g^T over the target points p of the correspondences, g = (0, z, -y,
    1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1).  -> float64 [6, 6] on the host (it arrives in the call's read-back); with
    return_correspondences also int64 CUDA [C, 2], rows (source row, target row) in ascending source row."""
    info, _, _, _, corr = _information(source, target, max_correspondence_distance, transformation,
                                       want_corr=return_correspondences)
    return (info, corr) if return_correspondences else info


def evaluate_registration(source, target, max_correspondence_distance, transformation=None):
    """Open3D's evaluate_registration on the GPU, from one rdm_information_matrix call: -> RegistrationResult(transformation,
    fitness = C / n_source, inlier_rmse = sqrt(sum d2 / C) (0 without correspondences), num_correspondences = C, iterations 0)
    with correspondence_set int64 CUDA [C, 2] and, as an extra attribute, `information` (float64 [6, 6])."""
    import math
    import numpy as np
    info, c, sum_d2, _, corr = _information(source, target, max_correspondence_distance, transformation, want_corr=True)
    n = source.shape[0]
    T = _transform_arg(transformation, 'transformation')
    res = RegistrationResult(np.eye(4) if T is None else T.copy(), c / n if n > 0 else 0.0, math.sqrt(sum_d2 / c) if c > 0 else 0.0,
                             c, 0, correspondence_set=corr)
    res.information = info
    return res


POSE_GRAPH_REPORT_WIDTH = 8  # per graph: initial cost, final cost, iterations, PCG iterations, stop reason, status, lambda, gradient
POSE_GRAPH_STOP = {1: 'gradient', 2: 'cost', 3: 'max_iterations', 4: 'empty'}
POSE_GRAPH_MAX_NODES, POSE_GRAPH_MAX_EDGES = 65536, 1048576  # per graph (rdm_pose_graph_optimize)
POSE_GRAPH_PRECONDITIONERS = {'block_jacobi': 0, 'chain': 1}  # rdm_pose_graph_optimize_pc's `preconditioner`
POSE_GRAPH_LINEAR_SOLVERS = {'pcg': 0, 'direct': 1}  # rdm_pose_graph_optimize_ls's `linear_solver`


class PoseGraphResult:
    """What pose_graph_optimize returns.  nodes: float64 [N, 4, 4] and weights: float64 [E] (the line-process weights l_e at the
    final poses; 1 for certain edges and without a line process) and pruned: bool [E] (uncertain edges with l_e <
    edge_prune_threshold; they stay in the arrays), on the device the call ran on; per graph, as host numpy arrays [G]:
    initial_cost, final_cost, iterations (accepted and rejected steps), pcg_iterations (in total), stop_reason (int: 1 the
    gradient test, 2 the cost test, 3 max_iterations, 4 a graph without nodes or edges; stop_reasons has the names), damping
    (the final lambda) and gradient_max (the largest gradient entry at the last linearisation)."""

    def __init__(self, nodes, weights, pruned, report):
        import numpy as np
        self.nodes, self.weights, self.pruned = nodes, weights, pruned
        rep = np.asarray(report, dtype=np.float64).reshape(-1, POSE_GRAPH_REPORT_WIDTH)
        self.initial_cost, self.final_cost = rep[:, 0].copy(), rep[:, 1].copy()
        self.iterations, self.pcg_iterations = rep[:, 2].astype(np.int64), rep[:, 3].astype(np.int64)
        self.stop_reason = rep[:, 4].astype(np.int64)
        self.stop_reasons = [POSE_GRAPH_STOP.get(int(v), 'none') for v in self.stop_reason]
        self.damping, self.gradient_max = rep[:, 6].copy(), rep[:, 7].copy()


def _pose_graph_connected(edges, node_offsets, edge_offsets, who='pose_graph_optimize'):
    """Union-find over every graph's edges: ValueError naming the first node that no path connects to its graph's node 0.
    Edges whose ends are outside their graph are left to the library's own check.  Graphs without edges are returned as given
    and are not checked."""
    for g in range(len(node_offsets) - 1):
        n, e0, e1 = int(node_offsets[g + 1] - node_offsets[g]), int(edge_offsets[g]), int(edge_offsets[g + 1])
        if n == 0 or e1 == e0:
            continue
        parent = list(range(n))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        for s, t in edges[e0:e1].tolist():
            if 0 <= s < n and 0 <= t < n:
                a, b = find(s), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
        for i in range(n):
            if find(i) != 0:
                raise ValueError(f'{who}: no path of edges connects node {i} of graph {g} to its node 0')


def _pose_graph_args(who, nodes, edges, transforms, informations, uncertain, graph_node_offsets, graph_edge_offsets, weights=None,
                     before_connectivity=None):
    """The arguments of a pose-graph call (pose_graph_optimize, pose_graph_marginals), checked and moved: nodes, transforms,
    informations (and weights, when given) float64 on the device of the first of them that lies on one (else the current device),
    edges / uncertain / offsets as host numpy arrays.  Every ValueError is raised before anything moves to a device: shapes, one row
    per edge, the offsets, a weight that is negative or not finite, whatever before_connectivity() raises, a node without a path to
    its graph's node 0.  -> (device, X, T, L, edges, uncertain, node offsets, edge offsets, G, weights)."""
    import numpy as np

    def f64(t, shape, name):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64)))
        if t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
            dims = ''.join(f', {d}' for d in shape)
            raise ValueError(f'{who}: {name} must be [*{dims}], got {tuple(t.shape)}')
        return t.detach()

    def host(t, dtype):
        if t is None:
            return None
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(t).astype(dtype, copy=False))

    X, T, Lm = f64(nodes, (4, 4), 'nodes'), f64(transforms, (4, 4), 'transforms'), f64(informations, (6, 6), 'informations')
    W = None if weights is None else f64(weights, (), 'weights')
    ed = host(edges, np.int64).reshape(-1, 2)
    unc = host(uncertain, np.uint8)
    n, e = X.shape[0], ed.shape[0]
    if T.shape[0] != e or Lm.shape[0] != e or (unc is not None and unc.shape != (e,)):
        raise ValueError(f'{who}: edges, transforms, informations and uncertain must have one row per edge')
    if W is not None and W.shape[0] != e:
        raise ValueError(f'{who}: weights must have one entry per edge, got {tuple(W.shape)}')
    if (graph_node_offsets is None) != (graph_edge_offsets is None):
        raise ValueError(f'{who}: graph_node_offsets and graph_edge_offsets go together')
    noff = np.array([0, n], np.int64) if graph_node_offsets is None else host(graph_node_offsets, np.int64)
    eoff = np.array([0, e], np.int64) if graph_edge_offsets is None else host(graph_edge_offsets, np.int64)
    if noff.ndim != 1 or noff.shape != eoff.shape or noff.shape[0] < 1 or noff[0] != 0 or eoff[0] != 0 or noff[-1] != n or eoff[-1] != e \
            or np.any(np.diff(noff) < 0) or np.any(np.diff(eoff) < 0):
        raise ValueError(f'{who}: offsets must be [G + 1], ascending, from 0 to the number of nodes / edges')
    if W is not None and e > 0 and not bool((torch.isfinite(W) & (W >= 0)).all()):
        raise ValueError(f'{who}: weights must be finite and >= 0')
    if before_connectivity is not None:
        before_connectivity()
    g = noff.shape[0] - 1
    if g > 0 and np.diff(noff).max() <= POSE_GRAPH_MAX_NODES and np.diff(eoff).max() <= POSE_GRAPH_MAX_EDGES:
        _pose_graph_connected(ed, noff, eoff, who)
    tensors = [t for t in (X, T, Lm) if t.is_cuda]
    dev = tensors[0].device if tensors else torch.device('cuda', torch.cuda.current_device())
    X, T, Lm = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (X, T, Lm))
    if W is not None:
        W = W.to(device=dev, dtype=torch.float64).contiguous()
    return dev, X, T, Lm, ed, unc, noff, eoff, g, W


def pose_graph_optimize(nodes, edges, transforms, informations, uncertain=None, *, line_process_weight=None,
                        edge_prune_threshold=0.25, max_iterations=100, gradient_tolerance=1e-9, cost_tolerance=1e-12,
                        graph_node_offsets=None, graph_edge_offsets=None, pcg_max_iterations=None, pcg_tolerance=1e-10,
                        preconditioner='block_jacobi', linear_solver='pcg'):
    """Pose-graph optimisation on the GPU (rdm_pose_graph_optimize; what Open3D's global_optimization does; parity unpinned,
    the definition is DESIGN.md section 7, pinned to tests/pose_graph_restatement.py).  nodes float64 [N, 4, 4] (the pose of scan i
    in the frame of its graph's node 0, which stays fixed), edges int64 [E, 2] rows (s, t) numbered inside their graph, transforms
    float64 [E, 4, 4] (source-scan to target-scan coordinates -- a pair's estimated_transform with src = s, ref = t; the model is
    X_s = X_t T), informations float64 [E, 6, 6] (rotation first, as ops.information_matrix), uncertain bool [E] (loop-closure
    edges; None: none).  Tensors (device or host) or anything numpy holds.  A batch of graphs is concatenated, with
    graph_node_offsets / graph_edge_offsets int64 [G + 1] (None: one graph).  line_process_weight None: every weight is 1;
    mu > 0: uncertain edges carry l = (mu / (mu + r^T L r))^2.  pcg_max_iterations None: 60 (N - 1) + 64 of the largest graph (ten times the unknowns: in float64 the conjugate gradients
    need a few times their exact-arithmetic count on these ill-conditioned systems; the tolerance ends them before; a graph of many
    thousands of nodes spends that inside one kernel launch with 'block_jacobi' -- pass a cap of your own there or choose 'chain',
    DESIGN.md section 7).  preconditioner: 'block_jacobi' (the default: the node blocks) or 'chain' (the block tridiagonal part of
    the system along the odometry chain, nodes i and i + 1, factored exactly: 7 to 17 times fewer conjugate-gradient iterations
    on drives with loop closures, each one longer -- docs/EXPERIMENTS.md 5o; same minimum within the tolerances, other bits); any
    other string is a ValueError.  linear_solver: 'pcg' (the default: the conjugate gradients above) or 'direct' (a direct sparse
    solve for a chain with loop closures, DESIGN.md section 7: one end of every off-chain edge is taken out, the rest is factored
    exactly along the chain, and the separator's dense Schur complement is factored in 6 x 6 blocks; preconditioner,
    pcg_max_iterations and pcg_tolerance are ignored and pcg_iterations is 0; a graph may need at most 256 separator nodes
    (rdm_pose_graph_direct_max_separator) -- above that the call is a RuntimeError naming the graph and the count, and nothing falls
    back to the conjugate gradients); any other string is a ValueError.
    -> PoseGraphResult.  ValueError for a node without a path to node 0; RuntimeError (the library's argument error, every output
    untouched) for a self edge, an index outside its graph, a non-finite entry, an asymmetric information matrix, a graph above
    65 536 nodes or 1 048 576 edges."""
    import numpy as np
    if preconditioner not in POSE_GRAPH_PRECONDITIONERS:
        raise ValueError(f'pose_graph_optimize: preconditioner must be one of {sorted(POSE_GRAPH_PRECONDITIONERS)}, got {preconditioner!r}')
    pre = POSE_GRAPH_PRECONDITIONERS[preconditioner]
    if linear_solver not in POSE_GRAPH_LINEAR_SOLVERS:
        raise ValueError(f'pose_graph_optimize: linear_solver must be one of {sorted(POSE_GRAPH_LINEAR_SOLVERS)}, got {linear_solver!r}')
    solver = POSE_GRAPH_LINEAR_SOLVERS[linear_solver]
    L = _lib.lib()

    def check_weight():
        if line_process_weight is not None and not line_process_weight > 0:
            raise ValueError(f'pose_graph_optimize: line_process_weight must be > 0 or None, got {line_process_weight}')

    dev, X, T, Lm, ed, unc, noff, eoff, g, _ = _pose_graph_args('pose_graph_optimize', nodes, edges, transforms, informations, uncertain,
                                                                graph_node_offsets, graph_edge_offsets, before_connectivity=check_weight)
    n, e = X.shape[0], ed.shape[0]
    if pcg_max_iterations is None:
        pcg_max_iterations = 60 * max(int(np.diff(noff).max()) - 1 if g > 0 else 0, 0) + 64
    out = torch.empty_like(X)
    weights = torch.empty(e, dtype=torch.float64, device=dev)
    pruned = torch.empty(e, dtype=torch.uint8, device=dev)
    report = np.zeros((g, POSE_GRAPH_REPORT_WIDTH), np.float64)
    with torch.cuda.device(dev):
        size = L.rdm_pose_graph_workspace_bytes_ls(g, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data, pre, solver)
        if size == 0 and solver == 0:  # (offsets the library refuses: the call below reports them, as it always did)
            size = L.rdm_pose_graph_workspace_bytes_pc(g, n, e, pre)
        elif size == 0:  # (an edge outside its graph, a graph above a limit: the library's message, before any GPU work)
            _lib.check(-1, 'rdm_pose_graph_optimize')
        ws = scratch(dev, size)
        _lib.check(L.rdm_pose_graph_optimize_ls(g, noff.ctypes.data, eoff.ctypes.data, _lib.ptr(X), ed.ctypes.data, _lib.ptr(T),
                                                _lib.ptr(Lm), 0 if unc is None else unc.ctypes.data,
                                                0.0 if line_process_weight is None else float(line_process_weight),
                                                float(edge_prune_threshold), int(max_iterations), float(gradient_tolerance),
                                                float(cost_tolerance), int(pcg_max_iterations), float(pcg_tolerance), pre, solver,
                                                _lib.ptr(out), _lib.ptr(weights), _lib.ptr(pruned), report.ctypes.data,
                                                ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_pose_graph_optimize')
    return PoseGraphResult(out, weights, pruned.bool(), report)


class PoseGraphMarginals:
    """What pose_graph_marginals returns.  covariances: float64 [N, 6, 6] on the device the call ran on -- row i is the covariance
    of node i's right perturbation X_i [Exp(dw) | dt] (rotation first) given its graph's node 0, whose row is zero; every block is
    exactly symmetric.  Per graph, host numpy [G]: status (0; 4: a pivot was not positive -- zero weights cut a node off, or an
    information matrix is indefinite -- and the graph's rows but row 0 are NaN) and separator (the direct solve's separator size)."""

    def __init__(self, covariances, report):
        import numpy as np
        self.covariances = covariances
        rep = np.asarray(report, dtype=np.float64).reshape(-1, 2)
        self.status, self.separator = rep[:, 0].astype(np.int64), rep[:, 1].astype(np.int64)


def pose_graph_marginals(nodes, edges, transforms, informations, weights=None, *, graph_node_offsets=None, graph_edge_offsets=None):
    """The marginal covariance of every pose of a pose graph on the GPU (rdm_pose_graph_marginals; g2o's computeMarginals, GTSAM's
    Marginals): Sigma_i = (H^-1)_ii with H = sum_e w_e J_e^T L_e J_e over the free nodes, the undamped
    Gauss-Newton matrix at `nodes` -- normally pose_graph_optimize's output, with its `weights` (float64 [E] >= 0, device or host;
    None: every weight 1; set pruned edges' to 0 to leave them out).  The other arguments are pose_graph_optimize's.  The blocks come
    from the direct solve's factors by a selected inversion (no dense inverse), so a graph may need at most 256 separator nodes:
    above that the call is a RuntimeError naming the graph and the count.  -> PoseGraphMarginals.  ValueError, before any library
    call, for shapes, offsets, a negative or non-finite weight and a node without a path to node 0; RuntimeError (the library's
    argument error, nothing written) for what pose_graph_optimize refuses and for a residual beyond the angle limit."""
    import numpy as np
    dev, X, T, Lm, ed, _, noff, eoff, g, W = _pose_graph_args('pose_graph_marginals', nodes, edges, transforms, informations, None,
                                                              graph_node_offsets, graph_edge_offsets, weights=weights)
    L = _lib.lib()
    n = X.shape[0]
    out = torch.empty((n, 6, 6), dtype=torch.float64, device=dev)
    report = np.zeros((g, 2), np.float64)
    with torch.cuda.device(dev):
        size = L.rdm_pose_graph_marginals_workspace_bytes(g, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data)
        if size == 0:  # (an edge outside its graph, a graph above a limit: the library's message, before any GPU work)
            _lib.check(-1, 'rdm_pose_graph_marginals')
        ws = scratch(dev, size)
        _lib.check(L.rdm_pose_graph_marginals(g, noff.ctypes.data, eoff.ctypes.data, _lib.ptr(X), ed.ctypes.data, _lib.ptr(T), _lib.ptr(Lm),
                                              0 if W is None else _lib.ptr(W), _lib.ptr(out), report.ctypes.data, ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr()), 'rdm_pose_graph_marginals')
    return PoseGraphMarginals(out, report)


class PoseGraphConsistency:
    """What pose_graph_consistency returns, float64 on the device the call ran on.  covariances [N, 6, 6]: pose_graph_marginals' output,
    bit for bit.  Per pair (s, t): cross [P, 6, 6] = Sigma_st (rows: s; zero with node 0), residual_covariances [P, 6, 6] = the
    covariance M of the pair's residual under the graph (exactly symmetric), d2 [P] = r^T (M + L^-1)^-1 r, pair_status uint8 [P] (0; 1: L
    or M + L^-1 is not positive definite, d2 is NaN).  Per graph, host numpy [G]: status (0; 4: the graph's rows and its pairs' are NaN)
    and separator, as PoseGraphMarginals'."""

    def __init__(self, covariances, cross, residual_covariances, d2, pair_status, report):
        import numpy as np
        self.covariances, self.cross, self.residual_covariances, self.d2, self.pair_status = covariances, cross, residual_covariances, d2, \
            pair_status
        rep = np.asarray(report, dtype=np.float64).reshape(-1, 2)
        self.status, self.separator = rep[:, 0].astype(np.int64), rep[:, 1].astype(np.int64)


def pose_graph_consistency(nodes, edges, transforms, informations, weights=None, *, pairs, pair_transforms=None, pair_informations=None,
                           graph_node_offsets=None, graph_edge_offsets=None, graph_pair_offsets=None):
    """Cross covariances of pairs of poses and the consistency of candidate edges with a pose graph on the GPU
    (rdm_pose_graph_consistency; g2o's computeMarginals with block pairs, GTSAM's jointMarginalCovariance).  The
    first five arguments and the node / edge offsets are pose_graph_marginals'.  pairs int64 [P, 2] rows (s, t) numbered inside their
    graph (graph_pair_offsets int64 [G + 1]; None: one graph), pair_transforms float64 [P, 4, 4] with an edge's convention X_s = X_t T
    (None: the current relative poses X_t^-1 X_s, formed in float64 on the device -- the result is then the covariance of the relative
    pose and d2 is 0 up to rounding), pair_informations float64 [P, 6, 6] or None (d2 = r^T M^-1 r).  d2 is the squared Mahalanobis
    distance of a measured edge from the graph's relative pose under the graph's uncertainty plus its own; it is only as calibrated as
    the information matrices are.  -> PoseGraphConsistency.  ValueError, before any library call, for what pose_graph_marginals raises
    and for the pairs' shape, offsets, s = t and a node outside its graph; RuntimeError (nothing written) for what the library
    refuses: pose_graph_marginals' cases, a non-finite pair transform or information, an asymmetric information, a pair residual
    beyond the angle limit."""
    import numpy as np
    who = 'pose_graph_consistency'

    def check_pairs():
        pr = np.asarray(pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
        if pr.ndim != 2 or pr.shape[1] != 2 or pr.dtype.kind not in 'iu':
            raise ValueError(f'{who}: pairs must be integers [*, 2], got {pr.dtype} {tuple(pr.shape)}')
        state['pairs'] = pr = np.ascontiguousarray(pr.astype(np.int64, copy=False))
        p = pr.shape[0]
        for t, shape, name in ((pair_transforms, (4, 4), 'pair_transforms'), (pair_informations, (6, 6), 'pair_informations')):
            got = None if t is None else tuple(t.shape) if hasattr(t, 'shape') else np.shape(t)
            if t is not None and got != (p,) + shape:
                raise ValueError(f'{who}: {name} must be [{p}, {shape[0]}, {shape[1]}] (one per pair), got {got}')
        n = np.asarray(nodes).shape[0] if not isinstance(nodes, torch.Tensor) else nodes.shape[0]
        if (graph_pair_offsets is None) != (graph_node_offsets is None):
            raise ValueError(f'{who}: graph_pair_offsets goes with graph_node_offsets and graph_edge_offsets')
        noff = np.array([0, n], np.int64) if graph_node_offsets is None else np.asarray(
            graph_node_offsets.cpu() if isinstance(graph_node_offsets, torch.Tensor) else graph_node_offsets, dtype=np.int64)
        poff = np.array([0, p], np.int64) if graph_pair_offsets is None else np.ascontiguousarray(np.asarray(
            graph_pair_offsets.cpu() if isinstance(graph_pair_offsets, torch.Tensor) else graph_pair_offsets, dtype=np.int64))
        if poff.ndim != 1 or poff.shape != noff.shape or poff[0] != 0 or poff[-1] != p or np.any(np.diff(poff) < 0):
            raise ValueError(f'{who}: graph_pair_offsets must be [G + 1], ascending, from 0 to the number of pairs')
        state['poff'] = poff
        size = np.repeat(np.diff(noff), np.diff(poff))
        same = np.nonzero(pr[:, 0] == pr[:, 1])[0]
        if len(same):
            raise ValueError(f'{who}: pair {same[0]} joins node {pr[same[0], 0]} to itself')
        out = np.nonzero((pr < 0).any(1) | (pr >= size[:, None]).any(1))[0]
        if len(out):
            k = out[0]
            raise ValueError(f'{who}: pair {k} ({pr[k, 0]}, {pr[k, 1]}) is outside its graph of {size[k]} nodes')

    state = {}
    dev, X, T, Lm, ed, _, noff, eoff, g, W = _pose_graph_args(who, nodes, edges, transforms, informations, None, graph_node_offsets,
                                                              graph_edge_offsets, weights=weights, before_connectivity=check_pairs)
    pr, poff = state['pairs'], state['poff']
    n, p = X.shape[0], pr.shape[0]

    def moved(t):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64)))
        return t.detach().to(device=dev, dtype=torch.float64).contiguous()

    if pair_transforms is None:  # X_t^-1 X_s with the closed-form inverse [R^T | -R^T t]
        glob = torch.from_numpy(pr + np.repeat(noff[:-1], np.diff(poff))[:, None]).to(dev)
        Xs, Xt = X[glob[:, 0]], X[glob[:, 1]]
        Rt = Xt[:, :3, :3].transpose(1, 2)
        PT = torch.zeros((p, 4, 4), dtype=torch.float64, device=dev)
        PT[:, :3, :3] = Rt @ Xs[:, :3, :3]
        PT[:, :3, 3] = (Rt @ (Xs[:, :3, 3] - Xt[:, :3, 3]).unsqueeze(2)).squeeze(2)
        PT[:, 3, 3] = 1.0
    else:
        PT = moved(pair_transforms)
    PL = None if pair_informations is None else moved(pair_informations)
    L = _lib.lib()
    cov = torch.empty((n, 6, 6), dtype=torch.float64, device=dev)
    cross, resid = (torch.empty((p, 6, 6), dtype=torch.float64, device=dev) for _ in range(2))
    d2 = torch.empty(p, dtype=torch.float64, device=dev)
    pstat = torch.empty(p, dtype=torch.uint8, device=dev)
    report = np.zeros((g, 2), np.float64)
    with torch.cuda.device(dev):
        size = L.rdm_pose_graph_consistency_workspace_bytes(g, noff.ctypes.data, eoff.ctypes.data, ed.ctypes.data, poff.ctypes.data,
                                                            pr.ctypes.data)
        if size == 0:  # (an edge outside its graph, a graph above a limit: the library's message, before any GPU work)
            _lib.check(-1, 'rdm_pose_graph_consistency')
        ws = scratch(dev, size)
        _lib.check(L.rdm_pose_graph_consistency(g, noff.ctypes.data, eoff.ctypes.data, _lib.ptr(X), ed.ctypes.data, _lib.ptr(T), _lib.ptr(Lm),
                                                0 if W is None else _lib.ptr(W), poff.ctypes.data, pr.ctypes.data, _lib.ptr(PT),
                                                0 if PL is None else _lib.ptr(PL), _lib.ptr(cov), _lib.ptr(cross), _lib.ptr(resid),
                                                _lib.ptr(d2), _lib.ptr(pstat), report.ctypes.data, ws.data_ptr(), ws.numel(),
                                                _lib.stream_ptr()), 'rdm_pose_graph_consistency')
    return PoseGraphConsistency(cov, cross, resid, d2, pstat, report)


def _gt_check(t, name, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f'gt_node_correspondences: {name} must be a tensor')
    if t.device != device:
        raise RuntimeError(f'gt_node_correspondences: {name} is on {t.device}, expected {device}')
    if t.dtype != dtype:
        raise RuntimeError(f'gt_node_correspondences: {name} has dtype {t.dtype}, expected {dtype}')
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'gt_node_correspondences: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t.contiguous()


def _gt_mask(t, name, shape, device):
    if t is None:
        return None
    if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return _gt_check(t, name, shape, torch.uint8, device)


def _gt_call(ref_nodes, src_nodes, ref_pts, ref_idx, src_pts, src_idx, k, transform, pos_radius, masks):
    L = _lib.lib()
    dev, m, n = ref_nodes.device, ref_nodes.shape[0], src_nodes.shape[0]
    cap = m * n  # the worst case B = M*N
    idx = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    ovl = torch.empty((cap,), dtype=torch.float32, device=dev)
    flags = torch.zeros((3,), dtype=torch.int32, device=dev)  # counts {C, B}, status
    ws = scratch(dev, L.rdm_gt_node_correspondences_workspace_bytes(m, n))
    _lib.check(L.rdm_gt_node_correspondences(ref_nodes.data_ptr(), m, src_nodes.data_ptr(), n, ref_pts.data_ptr(), _lib.ptr(ref_idx),
                                             0 if ref_idx is None else ref_pts.shape[0], src_pts.data_ptr(), _lib.ptr(src_idx),
                                             0 if src_idx is None else src_pts.shape[0], k, *[_lib.ptr(t) for t in masks],
                                             transform.data_ptr(), float(pos_radius), idx.data_ptr(), ovl.data_ptr(), cap,
                                             flags.data_ptr(), flags[2:].data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               'rdm_gt_node_correspondences')
    c, b, status = (int(v) for v in flags.cpu())
    if status != 0:  # (cannot happen with capacity M*N)
        raise RuntimeError('rdm_gt_node_correspondences: output capacity exceeded')
    return idx[:c], ovl[:c], b


def _gt_inputs(ref_nodes, src_nodes, transform):
    if not isinstance(ref_nodes, torch.Tensor) or ref_nodes.device.type != 'cuda':
        raise RuntimeError('gt_node_correspondences: ref_nodes must be a CUDA tensor')
    dev = ref_nodes.device
    m = ref_nodes.shape[0] if ref_nodes.dim() == 2 else -1
    n = src_nodes.shape[0] if isinstance(src_nodes, torch.Tensor) and src_nodes.dim() == 2 else -1
    if m <= 0 or n <= 0:
        raise RuntimeError(f'gt_node_correspondences: bad node shapes {tuple(ref_nodes.shape)} / {tuple(src_nodes.shape)}')
    return (dev, m, n, _gt_check(ref_nodes, 'ref_nodes', (m, 3), torch.float32, dev),
            _gt_check(src_nodes, 'src_nodes', (n, 3), torch.float32, dev), _gt_check(transform, 'transform', (4, 4), torch.float32, dev))


def gt_node_correspondences(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks=None,
                            src_masks=None, ref_knn_masks=None, src_knn_masks=None):
    """get_node_correspondences (geotransformer/modules/registration/matching.py:252-350) on device tensors:
    nodes f32 [M,3] / [N,3], gathered patch points f32 [M,K,3] / [N,K,3] (K <= 128), transform f32 [4,4] (src -> ref),
    masks bool / u8 or None (= all valid) -> (corr_indices i64 [C,2], corr_overlaps f32 [C]), the candidates with overlap > 0
    in (ref, src) order.  Synchronises the stream once (C is data dependent)."""
    dev, m, n, ref_nodes, src_nodes, transform = _gt_inputs(ref_nodes, src_nodes, transform)
    k = ref_knn_points.shape[1] if isinstance(ref_knn_points, torch.Tensor) and ref_knn_points.dim() == 3 else -1
    if not 0 < k <= 128:
        raise RuntimeError(f'gt_node_correspondences: ref_knn_points must be [M, K, 3] with 0 < K <= 128')
    ref_knn_points = _gt_check(ref_knn_points, 'ref_knn_points', (m, k, 3), torch.float32, dev)
    src_knn_points = _gt_check(src_knn_points, 'src_knn_points', (n, k, 3), torch.float32, dev)
    masks = [_gt_mask(ref_masks, 'ref_masks', (m,), dev), _gt_mask(src_masks, 'src_masks', (n,), dev),
             _gt_mask(ref_knn_masks, 'ref_knn_masks', (m, k), dev), _gt_mask(src_knn_masks, 'src_knn_masks', (n, k), dev)]
    idx, ovl, _ = _gt_call(ref_nodes, src_nodes, ref_knn_points, None, src_knn_points, None, k, transform, pos_radius, masks)
    return idx, ovl


def gt_node_correspondences_indexed(ref_nodes, src_nodes, ref_points, ref_knn_indices, src_points, src_knn_indices, transform,
                                    pos_radius, ref_masks=None, src_masks=None, ref_knn_masks=None, src_knn_masks=None):
    """gt_node_correspondences with the patches as point_to_node writes them: fine points f32 [n_r,3] / [n_s,3] and int64 slot
    indices [M,K] / [N,K] into them (an index outside [0, n) is the zero pad row, model.py:268-273) -> (corr_indices,
    corr_overlaps, B) with B the number of candidate patch pairs that passed the enclosing-sphere test."""
    dev, m, n, ref_nodes, src_nodes, transform = _gt_inputs(ref_nodes, src_nodes, transform)
    k = ref_knn_indices.shape[1] if isinstance(ref_knn_indices, torch.Tensor) and ref_knn_indices.dim() == 2 else -1
    if not 0 < k <= 128:
        raise RuntimeError(f'gt_node_correspondences: ref_knn_indices must be [M, K] with 0 < K <= 128')
    ref_points = _gt_check(ref_points, 'ref_points', (ref_points.shape[0], 3), torch.float32, dev)
    src_points = _gt_check(src_points, 'src_points', (src_points.shape[0], 3), torch.float32, dev)
    if ref_points.shape[0] == 0 or src_points.shape[0] == 0:
        raise RuntimeError('gt_node_correspondences: empty cloud')
    ref_knn_indices = _gt_check(ref_knn_indices, 'ref_knn_indices', (m, k), torch.int64, dev)
    src_knn_indices = _gt_check(src_knn_indices, 'src_knn_indices', (n, k), torch.int64, dev)
    masks = [_gt_mask(ref_masks, 'ref_masks', (m,), dev), _gt_mask(src_masks, 'src_masks', (n,), dev),
             _gt_mask(ref_knn_masks, 'ref_knn_masks', (m, k), dev), _gt_mask(src_knn_masks, 'src_knn_masks', (n, k), dev)]
    return _gt_call(ref_nodes, src_nodes, ref_points, ref_knn_indices, src_points, src_knn_indices, k, transform, pos_radius, masks)


# ---- descriptor matching (rdm_feature_match) ---------------------------------------------------------------------------

FEATURE_MATCH_MODES = {'nearest': 0, 'mutual': 1, 'bilateral': 2}


def _fm_feats(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda' or t.dtype != torch.float32 or t.dim() != 2:
        raise RuntimeError(f'feature_match: {name} must be a float32 CUDA tensor [rows, C]')
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def feature_nearest(a, b, both_sides=False, return_phase2=False):
    """rdm_feature_match: for every row of a [N, C] the index (int64 [N]) of its nearest row of b [M, C] and the distance
    (float32 [N]) -- the float64 brute-force answer, lowest index among equal distances; with both_sides also the same for the
    rows of b -> (nn_ab, dist_ab, nn_ba, dist_ba) (the last two None without both_sides)[, phase2_lines int32[2] device: the
    lines of a / b that took the float64 pass].  No synchronisation."""
    L = _lib.lib()
    a, b = _fm_feats(a, 'a'), _fm_feats(b, 'b')
    if a.device != b.device or a.shape[1] != b.shape[1]:
        raise RuntimeError(f'feature_match: a {tuple(a.shape)} on {a.device} against b {tuple(b.shape)} on {b.device}')
    dev, n, m, c = a.device, a.shape[0], b.shape[0], a.shape[1]
    nn_ab = torch.empty((n,), dtype=torch.int64, device=dev)
    d_ab = torch.empty((n,), dtype=torch.float32, device=dev)
    nn_ba = torch.empty((m,), dtype=torch.int64, device=dev) if both_sides else None
    d_ba = torch.empty((m,), dtype=torch.float32, device=dev) if both_sides else None
    phase2 = torch.zeros((2,), dtype=torch.int32, device=dev)
    ws = scratch(dev, L.rdm_feature_match_workspace_bytes(n, m, int(both_sides)))
    _lib.check(L.rdm_feature_match(a.data_ptr(), a.stride(0) if n > 1 else c, n, b.data_ptr(), b.stride(0) if m > 1 else c, m, c,
                                   int(both_sides), nn_ab.data_ptr(), d_ab.data_ptr(), _lib.ptr(nn_ba), _lib.ptr(d_ba),
                                   phase2.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_feature_match')
    return (nn_ab, d_ab, nn_ba, d_ba, phase2) if return_phase2 else (nn_ab, d_ab, nn_ba, d_ba)


def _feature_match(ref_feats, src_feats, mutual, bilateral):
    """-> (ref_corr_indices, src_corr_indices, feat_dists), device; one read-back (the count) under `mutual`."""
    L = _lib.lib()
    mode = 1 if mutual else 2 if bilateral else 0
    ref_feats, src_feats = _fm_feats(ref_feats, 'ref_feats'), _fm_feats(src_feats, 'src_feats')
    dev, n, m = ref_feats.device, ref_feats.shape[0], src_feats.shape[0]
    if n == 0 and mode != 2 and m > 0:  # (bilateral has the rows of src to match, to nothing: rdm_feature_match's error)
        return (torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.int64, device=dev),
                torch.empty((0,), dtype=torch.float32, device=dev))
    nn_ab, d_ab, nn_ba, d_ba = feature_nearest(ref_feats, src_feats, both_sides=mode != 0)
    cap = n + m if mode == 2 else n
    ri = torch.empty((cap,), dtype=torch.int64, device=dev)
    si = torch.empty((cap,), dtype=torch.int64, device=dev)
    dist = torch.empty((cap,), dtype=torch.float32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(L.rdm_feature_match_select(mode, nn_ab.data_ptr(), d_ab.data_ptr(), _lib.ptr(nn_ba), _lib.ptr(d_ba), n, m,
                                          ri.data_ptr(), si.data_ptr(), dist.data_ptr(), count.data_ptr(), _lib.stream_ptr()),
               'rdm_feature_match_select')
    if mode == 1:
        k = int(count.item())  # the number of mutual pairs is data dependent: the one read-back
        ri, si, dist = ri[:k], si[:k], dist[:k]
    return ri, si, dist


def feature_match(ref_feats, src_feats, mutual=False, bilateral=False):
    """extract_corr_indices_from_feats (geotransformer/utils/registration.py:222-255) on device tensors: features f32 [N, C] /
    [M, C], 1 <= C <= 1024 -> (ref_corr_indices, src_corr_indices) int64, in the reference's order: (arange(N), nn_ref);
    `mutual`: the i with nn_src[nn_ref[i]] == i, ascending; `bilateral` (ignored under mutual): ([arange(N), nn_src], [nn_ref,
    arange(M)]).  Nearest = the float64 brute-force answer with the lowest index among equal distances (rdm_feature_match).
    N = 0 gives empty outputs; M = 0 raises."""
    return _feature_match(ref_feats, src_feats, mutual, bilateral)[:2]


def feature_correspondences(ref_points, src_points, ref_feats, src_feats, mutual=False, bilateral=False, return_feat_dist=False):
    """extract_correspondences_from_feats (geotransformer/utils/registration.py:258-277), plus `bilateral`:
    -> [ref_corr_points, src_corr_points(, feat_dists)]; feat_dists = sqrt of the float64 sum of squared differences, rounded to
    float32."""
    ri, si, dist = _feature_match(ref_feats, src_feats, mutual, bilateral)
    out = [ref_points[ri], src_points[si]]
    if return_feat_dist:
        out.append(dist)
    return out


# ---- offline evaluator (rdm_eval_pairs) ------------------------------------------------------------------------------

class PackedEvalPairs:
    """A batch of saved pairs as rdm_eval_pairs reads it: one host buffer (`buf`, uint8) holding every array at a 256-byte
    aligned offset (`sections`: name -> (offset, dtype, shape)), so that the batch costs one host-to-device copy.  Built by
    `pack_eval_pairs`, on any thread: nothing here touches the GPU."""

    def __init__(self, buf, sections, corr_offsets, num_pairs):
        self.buf, self.sections, self.corr_offsets, self.num_pairs = buf, sections, corr_offsets, num_pairs


def pack_eval_pairs(pairs, pin=None):
    """pairs: a list of dicts with the arrays of a test.py pair file (numpy or tensors): ref_corr_points, src_corr_points
    [C, 3], corr_scores [C], transform [4, 4], estimated_transform [4, 4] (optional: identity), ref_node_corr_indices,
    src_node_corr_indices, gt_node_corr_indices [G, 2], and the superpoint counts as ref_points_c / src_points_c (arrays, only
    their length is used) or node_dims = (M, N).  pin: page-locked buffer (default: when a GPU is present)."""
    import numpy as np

    def host(v, dtype):
        v = v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)
        return np.ascontiguousarray(v, dtype=dtype)

    P = len(pairs)
    ref = [host(d['ref_corr_points'], np.float32).reshape(-1, 3) for d in pairs]
    src = [host(d['src_corr_points'], np.float32).reshape(-1, 3) for d in pairs]
    sc = [host(d['corr_scores'], np.float32).reshape(-1) for d in pairs]
    rn = [host(d['ref_node_corr_indices'], np.int64).reshape(-1) for d in pairs]
    sn = [host(d['src_node_corr_indices'], np.int64).reshape(-1) for d in pairs]
    gn = [host(d['gt_node_corr_indices'], np.int64).reshape(-1, 2) for d in pairs]
    for p in range(P):
        if not (len(ref[p]) == len(src[p]) == len(sc[p])) or len(rn[p]) != len(sn[p]):
            raise ValueError(f'pair {p}: correspondence arrays of different lengths')
    dims = np.zeros((P, 2), np.int64)
    for p, d in enumerate(pairs):
        dims[p] = d['node_dims'] if 'node_dims' in d else (len(d['ref_points_c']), len(d['src_points_c']))
    eye = np.eye(4, dtype=np.float32)
    arrays = {
        'corr_offsets': np.concatenate([[0], np.cumsum([len(a) for a in sc])]).astype(np.int64),
        'node_offsets': np.concatenate([[0], np.cumsum([len(a) for a in rn])]).astype(np.int64),
        'gt_offsets': np.concatenate([[0], np.cumsum([len(a) for a in gn])]).astype(np.int64),
        'node_dims': dims,
        'gt_transform': np.stack([host(d['transform'], np.float32).reshape(4, 4) for d in pairs]) if P else np.zeros((0, 4, 4), np.float32),
        'est_transform': np.stack([host(d.get('estimated_transform', eye), np.float32).reshape(4, 4) for d in pairs])
        if P else np.zeros((0, 4, 4), np.float32),
        'ref_corr': np.concatenate(ref) if P else np.zeros((0, 3), np.float32),
        'src_corr': np.concatenate(src) if P else np.zeros((0, 3), np.float32),
        'corr_scores': np.concatenate(sc) if P else np.zeros((0,), np.float32),
        'ref_node_corr': np.concatenate(rn) if P else np.zeros((0,), np.int64),
        'src_node_corr': np.concatenate(sn) if P else np.zeros((0,), np.int64),
        'gt_node_corr': np.concatenate(gn) if P else np.zeros((0, 2), np.int64),
    }
    sections, off = {}, 0
    for name, a in arrays.items():
        sections[name] = (off, a.dtype, a.shape)
        off += (a.nbytes + 255) // 256 * 256
    if pin is None:
        pin = torch.cuda.is_available()
    buf = torch.empty(max(off, 256), dtype=torch.uint8, pin_memory=bool(pin))
    view = buf.numpy()
    for name, a in arrays.items():
        o = sections[name][0]
        view[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return PackedEvalPairs(buf, sections, arrays['corr_offsets'], P)


def evaluate_pairs(pairs, method='lgr', num_corr=None, *, acceptance_radius=0.6, distance_threshold=0.3, ransac_n=4,
                   num_iterations=50000, seed=0, device=None):
    """experiments/eval.py:100-239 for a batch of saved pairs on the GPU (rdm_eval_pairs): `pairs` is a list of per-pair dicts
    (pack_eval_pairs) or a PackedEvalPairs.  -> (records float64 [P, EVAL_RECORD_WIDTH] numpy, fields _lib.EVAL_FIELDS;
    transforms float32 [P, 4, 4] numpy: the registration the method used).  One host-to-device copy, a fixed number of launches,
    one device-to-host copy (which is the only synchronisation)."""
    import numpy as np
    L = _lib.lib()
    opts = _lib.EvalOptions.of(method, num_corr, acceptance_radius, distance_threshold, ransac_n, num_iterations, seed)
    if num_corr is not None and int(num_corr) <= 0:
        raise ValueError('num_corr must be positive')
    packed = pairs if isinstance(pairs, PackedEvalPairs) else pack_eval_pairs(pairs)
    P = packed.num_pairs
    W = _lib.EVAL_RECORD_WIDTH
    if P == 0:
        return np.zeros((0, W), np.float64), np.zeros((0, 4, 4), np.float32)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        d_in = packed.buf.to(dev, non_blocking=True)
        base = d_in.data_ptr()
        at = {name: base + o for name, (o, _, _) in packed.sections.items()}
        offs = packed.corr_offsets
        counts = np.diff(offs)
        out = torch.empty(P * W * 8 + P * 64, dtype=torch.uint8, device=dev)  # records, then the transforms
        rec_ptr, est_ptr = out.data_ptr(), out.data_ptr() + P * W * 8
        _lib.check(L.rdm_copy_device(est_ptr, at['est_transform'], P * 64, _lib.stream_ptr()), 'rdm_copy_device')
        ws = scratch(dev, L.rdm_eval_pairs_workspace_bytes(P, int(offs[-1]), int(counts.max()), ctypes.addressof(opts)))
        _lib.check(L.rdm_eval_pairs(P, at['corr_offsets'], offs.ctypes.data, at['ref_corr'], at['src_corr'], at['corr_scores'],
                                    at['gt_transform'], est_ptr, at['node_offsets'], at['ref_node_corr'], at['src_node_corr'],
                                    at['gt_offsets'], at['gt_node_corr'], at['node_dims'], ctypes.addressof(opts), rec_ptr,
                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr()), 'rdm_eval_pairs')
        h = out.cpu().numpy()
    records = h[:P * W * 8].view(np.float64).reshape(P, W).copy()
    transforms = h[P * W * 8:].view(np.float32).reshape(P, 4, 4).copy()
    if records[:, _lib.EVAL_FIELDS.index('bad_indices')].any():
        raise RuntimeError('rdm_eval_pairs: superpoint correspondence indices outside the pair\'s M x N nodes')
    return records, transforms
