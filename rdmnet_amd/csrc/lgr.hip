// a15/a16 -- dense correspondence extraction and local-to-global registration, entirely on the GPU.
//
// Reference: geotransformer/modules/geotransformer/local_global_registration.py:49-91
// (compute_correspondence_matrix), :145-202 (local_to_global_registration), :93-136 (convert_to_batch),
// geotransformer/modules/registration/procrustes.py:6-73 (weighted Kabsch; the reference moves H to the CPU for
// torch.svd -- here nothing leaves the device).  rdm_lgr is the configuration the reference ships (k = 1, dustbin,
// non-mutual, no limit) with an extraction kernel of its own; rdm_lgr_options takes every key of cfg.fine_matching
// (top-k, mutual, dustbin or confidence threshold, global score, correspondence limit).
//
// Stages (one launch each, sizes stay on the device):
//   extract   per patch: S = exp(log scores); row/column top-k incl. dustbin; keep (i,j) iff it beats
//             the dustbin (or the threshold) from either side (mutual: both) and both points are valid;
//             list them row-major (the order of torch.nonzero)                             :204-243
//   layout    exclusive scan of the per-patch counts, chunk list = patches with >= 3 matches
//   gather    stacked correspondences (ref point, src point, score) in patch order
//   limit     (correspondence_limit only) the L best-scored correspondences, in place order: the verification set  :152-160
//   local     per chunk: weighted Procrustes                                               :175-181
//   score     per chunk: #correspondences (of the verification set) with residual < acceptance radius :182-187
//   refine    first argmax, then 1 + (steps-1) global Procrustes rounds                    :188-200
// The rotation is obtained with Horn's quaternion form of the Kabsch problem (largest eigenvector of
// a symmetric 4x4, Jacobi in fp64): identical to V diag(1,1,det) U^T wherever that is unique, and
// the identity for a zero covariance like torch.svd.  Sums are accumulated in fp64.
#include "../../include/rdmnet_hip.h"
#include "common.h"
#include "procrustes.h"
#include "lockstep.h"

namespace {

using namespace rdm;

constexpr int kSide = 128;           // points per patch
constexpr int kPerPatch = 2 * kSide; // upper bound of matches per patch (one per row + one per column)

struct LgrBuffers {
  int32_t* patch_count;   // [B]
  int32_t* patch_offset;  // [B]
  int32_t* chunk_patch;   // [B]
  int32_t* meta;          // [0] = C, [1] = number of chunks, [2] = best chunk, [3] = size of the verification set (limit only)
  int32_t* local_i;       // [B, stride]
  int32_t* local_j;       // [B, stride]
  float* local_s;         // [B, stride]
  float* chunk_T;         // [B, 12]
  int32_t* chunk_inliers; // [B]
  int stride;             // matches a patch can hold: kPerPatch, or min(2 k K, K K) for top-k
  float* ver_ref;         // verification set [min(L, B stride)] of correspondence_limit = L; null: all correspondences
  float* ver_src;
  float* ver_s;
};

// cfg.fine_matching as the extraction kernel reads it
struct LgrSelect {
  int k, mutual, dustbin, global;
  float threshold;
};

// ------------------------------------------------------------------------------------------ extract
// Only the block of REAL rows and columns (+ the dustbin line of each side) is staged: a masked line of the Sinkhorn output
// holds fl(-1e12), i.e. exp() = 0 exactly, while a real row (column) of exp(scores) sums to 1, so its maximum is positive
// and a masked entry never wins nor ties a top-1 -- the compacted search returns the indices of the full 129 x 129 one.  A
// patch holds a few dozen real points of 128: 1-2 k exponentials per patch instead of 16.6 k.
__device__ __forceinline__ void lgr_extract_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* log_scores, int side,
                                                          const unsigned char* ref_mask,
                                                          const unsigned char* src_mask, LgrBuffers w) {
  (void)blockIdx; (void)gridDim;
  extern __shared__ float S[];  // compacted [(nr+1)][(nc+1)], row stride ldc (odd)
  __shared__ int rows[kSide + 1], cols[kSide + 1];  // original index of every compacted line, dustbin (= side) last
  __shared__ int rowarg[kSide + 1], colarg[kSide + 1];
  __shared__ unsigned char rowok[kSide + 1], colok[kSide + 1];
  __shared__ int rowcnt[kSide + 1];
  __shared__ int s_n[2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n1 = side + 1;
  const float* L = log_scores + static_cast<int64_t>(b) * n1 * n1;
  if (wave < 2) {  // wavefront 0: the real rows, wavefront 1: the real columns, ascending (ballot compaction)
    const unsigned char* mk = (wave == 0 ? ref_mask : src_mask) + static_cast<int64_t>(b) * side;
    int* list = wave == 0 ? rows : cols;
    int cnt = 0;
    for (int i0 = 0; i0 < side; i0 += 64) {
      const int i = i0 + lane;
      const bool on = i < side && mk[i] != 0;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(on);
      if (on) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = i;
      cnt += __popcll(bal);
    }
    if (lane == 0) {
      list[cnt] = side;
      s_n[wave] = cnt;
    }
  }
  __syncthreads();
  const int nr = s_n[0], nc = s_n[1], R = nr + 1, C = nc + 1, ldc = C | 1;
  for (int t = tid; t < R * C; t += 256) {
    const int r = t / C, c = t % C;
    S[r * ldc + c] = expf(L[static_cast<int64_t>(rows[r]) * n1 + cols[c]]);
  }
  __syncthreads();
  if (tid < nr) {  // top-1 of a real row over the real columns + dustbin (first maximum), must beat the dustbin column
    const int r = tid;
    float best = S[r * ldc];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = S[r * ldc + c];
      if (v > best) {
        best = v;
        arg = c;
      }
    }
    rowarg[r] = arg;  // compacted column (nc = dustbin)
    rowok[r] = (arg < nc && best > S[r * ldc + nc]) ? 1 : 0;
  } else if (tid >= 128 && tid < 128 + nc) {  // top-1 of a real column over the real rows + dustbin
    const int c = tid - 128;
    float best = S[c];
    int arg = 0;
    for (int r = 1; r < R; ++r) {
      const float v = S[r * ldc + c];
      if (v > best) {
        best = v;
        arg = r;
      }
    }
    colarg[c] = arg;
    colok[c] = (arg < nr && best > S[nr * ldc + c]) ? 1 : 0;
  }
  __syncthreads();
  auto is_corr = [&](int r, int c) { return (rowok[r] && rowarg[r] == c) || (colok[c] && colarg[c] == r); };
  if (tid < nr) {
    int cn = 0;
    for (int c = 0; c < nc; ++c) cn += is_corr(tid, c) ? 1 : 0;
    rowcnt[tid] = cn;
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int r = 0; r < nr; ++r) {
      const int cn = rowcnt[r];
      rowcnt[r] = acc;
      acc += cn;
    }
    w.patch_count[b] = acc;
  }
  __syncthreads();
  if (tid < nr) {  // row-major over the original indices (the order of torch.nonzero): the lists are ascending
    int pos = rowcnt[tid];
    for (int c = 0; c < nc; ++c)
      if (is_corr(tid, c)) {
        const int64_t o = static_cast<int64_t>(b) * kPerPatch + pos++;
        w.local_i[o] = rows[tid];
        w.local_j[o] = cols[c];
        w.local_s[o] = S[tid * ldc + c];
      }
  }
}

// ------------------------------------------------------------------------------------------ extract, every option
// The k-th element (1 <= k < n) of a staged line base[0], base[stride], .. in the order (value descending, index ascending)
// -- torch.topk's set with the lowest index kept among equal values at the boundary: element (v, j) of the line is among the
// k first iff v > t or (v == t and j <= jt).  One thread per line, k passes, each the first maximum behind the previous pick
// (k is 1-3 in practice: 3 x 129 LDS reads; the worst case, k = 128, is 129 x 128).
__device__ void lgr_kth(const float* base, int stride, int n, int k, float& t, int& jt) {
  float pv = 0.f;
  int pj = -1;
  for (int pass = 0; pass < k; ++pass) {
    float bv = -1.f;  // (the entries are exp() >= 0)
    int bj = -1;
    for (int c = 0; c < n; ++c) {
      const float v = base[c * stride];
      const bool behind = pass == 0 || v < pv || (v == pv && c > pj);
      if (behind && v > bv) {
        bv = v;
        bj = c;
      }
    }
    pv = bv;
    pj = bj;
  }
  t = pv;
  jt = pj;
}

// compute_correspondence_matrix for any k, mutual or not, dustbin or confidence threshold (:49-91), and the scores of :229-237.
// As above only the block of real rows and columns (+ the dustbin line with use_dustbin) is staged: a masked entry is exactly 0,
// and an entry equal to 0 passes neither test (the dustbin entry and the threshold are >= 0), so a line's top-k over the block
// decides every entry that can pass like the top-k over the full line; with k >= the staged length every staged entry is in it.
__device__ __forceinline__ void lgr_extract_topk_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* log_scores, int n1,
                                                               int side, const unsigned char* ref_mask, const unsigned char* src_mask,
                                                               const float* global_scores, LgrSelect o, LgrBuffers w) {
  (void)blockIdx; (void)gridDim;
  extern __shared__ float S[];  // compacted [(nr+D)][(nc+D)], D = 1 with the dustbin, row stride ldc (odd); static LDS stays < 4 KB (rdm::kMaxDynamicLds)
  __shared__ int rows[kSide + 1], cols[kSide + 1];  // original index of every compacted line, dustbin (= side) last
  __shared__ float rowt[kSide], colt[kSide];        // a line's k-th value and its index (lgr_kth)
  __shared__ int rowj[kSide], colj[kSide];
  __shared__ int rowcnt[kSide + 1];
  __shared__ int s_n[2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* L = log_scores + static_cast<int64_t>(b) * n1 * n1;
  if (wave < 2) {  // wavefront 0: the real rows, wavefront 1: the real columns, ascending (ballot compaction)
    const unsigned char* mk = (wave == 0 ? ref_mask : src_mask) + static_cast<int64_t>(b) * side;
    int* list = wave == 0 ? rows : cols;
    int cnt = 0;
    for (int i0 = 0; i0 < side; i0 += 64) {
      const int i = i0 + lane;
      const bool on = i < side && mk[i] != 0;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(on);
      if (on) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = i;
      cnt += __popcll(bal);
    }
    if (lane == 0) {
      list[cnt] = side;
      s_n[wave] = cnt;
    }
  }
  __syncthreads();
  const int D = o.dustbin ? 1 : 0;
  const int nr = s_n[0], nc = s_n[1], R = nr + D, C = nc + D, ldc = C | 1;
  for (int t = tid; t < R * C; t += 256) {
    const int r = t / C, c = t % C;
    S[r * ldc + c] = expf(L[static_cast<int64_t>(rows[r]) * n1 + cols[c]]);
  }
  __syncthreads();
  if (tid < nr) {  // a real row over the real columns (+ dustbin)
    const int r = tid;
    float t = -1.f;  // k >= C: every staged entry is among the k first
    int j = C;
    if (o.k < C) lgr_kth(S + r * ldc, 1, C, o.k, t, j);
    rowt[r] = t;
    rowj[r] = j;
  } else if (tid >= 128 && tid < 128 + nc) {  // a real column over the real rows (+ dustbin)
    const int c = tid - 128;
    float t = -1.f;
    int j = R;
    if (o.k < R) lgr_kth(S + c, ldc, R, o.k, t, j);
    colt[c] = t;
    colj[c] = j;
  }
  __syncthreads();
  auto is_corr = [&](int r, int c) {
    const float v = S[r * ldc + c];  // must exceed the line's dustbin entry, or the threshold
    const bool from_ref = (v > rowt[r] || (v == rowt[r] && c <= rowj[r])) && v > (D ? S[r * ldc + nc] : o.threshold);
    const bool from_src = (v > colt[c] || (v == colt[c] && r <= colj[c])) && v > (D ? S[nr * ldc + c] : o.threshold);
    return o.mutual ? (from_ref && from_src) : (from_ref || from_src);
  };
  if (tid < nr) {
    int cn = 0;
    for (int c = 0; c < nc; ++c) cn += is_corr(tid, c) ? 1 : 0;
    rowcnt[tid] = cn;
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int r = 0; r < nr; ++r) {
      const int cn = rowcnt[r];
      rowcnt[r] = acc;
      acc += cn;
    }
    w.patch_count[b] = acc < w.stride ? acc : w.stride;  // (acc <= min(k (nr + nc), nr nc) <= stride)
  }
  __syncthreads();
  if (tid < nr) {  // row-major over the original indices (the order of torch.nonzero): the lists are ascending
    const float gs = o.global ? global_scores[b] : 1.f;
    int pos = rowcnt[tid];
    for (int c = 0; c < nc; ++c)
      if (is_corr(tid, c) && pos < w.stride) {
        const int64_t oo = static_cast<int64_t>(b) * w.stride + pos++;
        w.local_i[oo] = rows[tid];
        w.local_j[oo] = cols[c];
        const float v = S[tid * ldc + c];
        w.local_s[oo] = o.global ? v * gs : v;  // (after the test, which never sees the global score: :229-237)
      }
  }
}

// ------------------------------------------------------------------------------------------ layout
// One wavefront: exclusive prefix of the per-patch correspondence counts (= offsets in nonzero order) and the
// ordered list of patches with >= min_corr correspondences.  Lane l owns patches 4l .. 4l+3 of each 256-patch chunk.
__device__ __forceinline__ void lgr_layout_kernel_body(const dim3 blockIdx, const dim3 gridDim, int batch, int min_corr, LgrBuffers w) {
  (void)blockIdx; (void)gridDim;
  const int lane = threadIdx.x;
  int acc = 0, chunks = 0;  // running totals, identical in all lanes
  for (int base = 0; base < batch; base += 256) {
    int c[4], local = 0, nbig = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = base + 4 * lane + u;
      c[u] = b < batch ? w.patch_count[b] : 0;
      local += c[u];
      nbig += (b < batch && c[u] >= min_corr) ? 1 : 0;
    }
    int inc = local, inb = nbig;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64), tb = __shfl_up(inb, o, 64);
      if (lane >= o) {
        inc += t;
        inb += tb;
      }
    }
    int off = acc + inc - local, slot = chunks + inb - nbig;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = base + 4 * lane + u;
      if (b < batch) {
        w.patch_offset[b] = off;
        off += c[u];
        if (c[u] >= min_corr) w.chunk_patch[slot++] = b;
      }
    }
    acc += __shfl(inc, 63, 64);
    chunks += __shfl(inb, 63, 64);
  }
  if (lane == 0) {
    w.meta[0] = acc;
    w.meta[1] = chunks;
    w.meta[2] = -1;
  }
}

__device__ __forceinline__ void lgr_gather_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* ref_knn, const float* src_knn, int side, LgrBuffers w,
                                  float* ref_corr, float* src_corr, float* corr_scores) {
  (void)blockIdx; (void)gridDim;
  const int b = blockIdx.x;
  const int cnt = w.patch_count[b], off = w.patch_offset[b];
  for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
    const int64_t o = static_cast<int64_t>(b) * w.stride + t;
    const float* r = ref_knn + (static_cast<int64_t>(b) * side + w.local_i[o]) * 3;
    const float* s = src_knn + (static_cast<int64_t>(b) * side + w.local_j[o]) * 3;
    for (int d = 0; d < 3; ++d) {
      ref_corr[3 * (off + t) + d] = r[d];
      src_corr[3 * (off + t) + d] = s[d];
    }
    corr_scores[off + t] = w.local_s[o];
  }
}

// ------------------------------------------------------------------------------------------ limit
// correspondence_limit = L (:152-160): the verification set is the L best-scored of the C correspondences -- the first L in the
// order (score descending, position ascending) -- kept in position order.  One workgroup, C only known here: an 8-bit radix
// select on the keys finds the L-th score (4 histogram passes, integer LDS atomics), then one ordered pass keeps what is above
// it and the first `need` positions equal to it.  C <= L: every correspondence, copied.
constexpr int kLimitThreads = 1024;
__device__ __forceinline__ void lgr_limit_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* ref_corr, const float* src_corr,
                                                        const float* scores, int limit, LgrBuffers w) {
  (void)blockIdx; (void)gridDim;
  __shared__ int hist[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_need;
  __shared__ int wsum[2][kLimitThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = w.meta[0];
  const bool all = C <= limit;
  unsigned prefix = 0;
  int need = limit;  // rank of the L-th score among the keys that share `prefix` above the current digit
  if (!all) {
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned above = shift == 24 ? 0u : ~0u << (shift + 8);
      for (int i = tid; i < C; i += kLimitThreads) {
        const unsigned key = order_key(scores[i]);
        if ((key & above) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      if (wave == 0) {  // lane l owns digits 255 - 4l .. 252 - 4l: the digit that holds the need-th key from the top
        int h[4], local = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          h[u] = hist[255 - 4 * lane - u];
          local += h[u];
        }
        int inc = local;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(inc, o, 64);
          if (lane >= o) inc += t;
        }
        int before = inc - local;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (before < need && need <= before + h[u]) {
            s_prefix = prefix | (static_cast<unsigned>(255 - 4 * lane - u) << shift);
            s_need = need - before;
          }
          before += h[u];
        }
      }
      __syncthreads();
      prefix = s_prefix;
      need = s_need;
    }
  }
  int base_g = 0, base_e = 0;  // correspondences above / equal to the L-th score before this tile (identical in all threads)
  for (int i0 = 0; i0 < C; i0 += kLimitThreads) {
    const int i = i0 + tid;
    bool g = false, e = false;
    if (i < C) {
      const unsigned key = order_key(scores[i]);
      g = all || key > prefix;
      e = !all && key == prefix;
    }
    const unsigned long long bg = __builtin_amdgcn_ballot_w64(g), be = __builtin_amdgcn_ballot_w64(e);
    const unsigned long long lower = (1ull << lane) - 1ull;
    if (lane == 0) {
      wsum[0][wave] = __popcll(bg);
      wsum[1][wave] = __popcll(be);
    }
    __syncthreads();
    int og = __popcll(bg & lower), oe = __popcll(be & lower), tg = 0, te = 0;
    for (int v = 0; v < kLimitThreads / 64; ++v) {
      const int a = wsum[0][v], c = wsum[1][v];
      if (v < wave) {
        og += a;
        oe += c;
      }
      tg += a;
      te += c;
    }
    const int eq_before = base_e + oe;
    if (g || (e && eq_before < need)) {
      const int dst = base_g + og + (eq_before < need ? eq_before : need);
      for (int d = 0; d < 3; ++d) {
        w.ver_ref[3 * dst + d] = ref_corr[3 * i + d];
        w.ver_src[3 * dst + d] = src_corr[3 * i + d];
      }
      w.ver_s[dst] = scores[i];
    }
    base_g += tg;
    base_e += te;
    __syncthreads();
  }
  if (tid == 0) w.meta[3] = all ? C : limit;
}

// ------------------------------------------------------------------------------------------ Procrustes
// Sum N values per thread over the block (fixed order); red must hold N * 16 doubles.
template <int N>
__device__ void block_sum_n(double (&v)[N], double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < N; ++k) red[k * 16 + wv] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[k * 16 + i];
    v[k] = t;
  }
}

// Weighted rigid fit src -> ref over entries [x0, x1) (procrustes.py:36-73).  Every thread of the
// block must call it; T (3x4, row-major R|t) is valid in all threads on return.
__device__ void block_procrustes(const float* src, const float* ref, const float* wts, const unsigned char* gate,
                                 int x0, int x1, double* red, double T[12], double (*basis)[4] = nullptr) {
  double sw = 0.0;
  for (int i = x0 + threadIdx.x; i < x1; i += blockDim.x) {
    float w = wts[i];
    if (gate && !gate[i]) w = 0.f;
    if (w < 0.f) w = 0.f;  // weight_thresh = 0
    sw += w;
  }
  {
    double t[1] = {sw};
    block_sum_n<1>(t, red);
    sw = t[0] + 1e-5;
  }
  const double inv_sw = 1.0 / sw;  // one fp64 division per fit instead of one per correspondence and pass
  double cs[3] = {0, 0, 0}, cr[3] = {0, 0, 0};
  for (int i = x0 + threadIdx.x; i < x1; i += blockDim.x) {
    float w = wts[i];
    if ((gate && !gate[i]) || w < 0.f) w = 0.f;
    const double wn = w * inv_sw;
    for (int d = 0; d < 3; ++d) {
      cs[d] += wn * src[3 * i + d];
      cr[d] += wn * ref[3 * i + d];
    }
  }
  {
    double t[6] = {cs[0], cs[1], cs[2], cr[0], cr[1], cr[2]};
    block_sum_n<6>(t, red);
    for (int d = 0; d < 3; ++d) {
      cs[d] = t[d];
      cr[d] = t[3 + d];
    }
  }
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // H[a][b] = sum w (s_a - cs_a)(r_b - cr_b)
  for (int i = x0 + threadIdx.x; i < x1; i += blockDim.x) {
    float w = wts[i];
    if ((gate && !gate[i]) || w < 0.f) w = 0.f;
    const double wn = w * inv_sw;
    double s[3], r[3];
    for (int d = 0; d < 3; ++d) {
      s[d] = src[3 * i + d] - cs[d];
      r[d] = ref[3 * i + d] - cr[d];
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) H[3 * a + b] += wn * s[a] * r[b];
  }
  block_sum_n<9>(H, red);
  const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7],
               Szz = H[8];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double q[4] = {1.0, 0.0, 0.0, 0.0};
  bool zero = true;  // no weight at all (a refinement step without inliers): the identity, as torch.svd of a zero matrix
                     // gives -- every frame is an eigenframe of N = 0, the carried one would return an arbitrary rotation
  for (int k = 0; k < 9; ++k) zero = zero && H[k] == 0.0;
  if (!zero) horn_quaternion(N, q, basis);
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  double R[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw),     2 * (qx * qz + qy * qw),
                 2 * (qx * qy + qz * qw),     1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                 2 * (qx * qz - qy * qw),     2 * (qy * qz + qx * qw),     1 - 2 * (qx * qx + qy * qy)};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) T[4 * a + b] = R[3 * a + b];
    T[4 * a + 3] = cr[a] - (R[3 * a] * cs[0] + R[3 * a + 1] * cs[1] + R[3 * a + 2] * cs[2]);
  }
}

// residual < radius in the reference's fp32 arithmetic (apply_transform + linalg.norm)
__device__ __forceinline__ bool is_inlier(const float* T, const float* src, const float* ref, int i, float radius) {
  const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
  const float ax = fmaf(z, T[2], fmaf(y, T[1], x * T[0])) + T[3];
  const float ay = fmaf(z, T[6], fmaf(y, T[5], x * T[4])) + T[7];
  const float az = fmaf(z, T[10], fmaf(y, T[9], x * T[8])) + T[11];
  const float dx = ref[3 * i] - ax, dy = ref[3 * i + 1] - ay, dz = ref[3 * i + 2] - az;
  return __fsqrt_rn((dx * dx + dy * dy) + dz * dz) < radius;
}

// one block per chunk: local Procrustes, then inlier count over ALL correspondences (of the verification set)
__device__ __forceinline__ void lgr_local_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* ref_corr, const float* src_corr,
                                                        const float* scores, float radius, LgrBuffers w) {
  (void)blockIdx; (void)gridDim;
  __shared__ double red[9 * 16];
  __shared__ float Tf[12];
  __shared__ int cnt_sh;
  const int chunk = blockIdx.x;
  if (chunk >= w.meta[1]) return;
  const int b = w.chunk_patch[chunk];
  const int x0 = w.patch_offset[b], x1 = x0 + w.patch_count[b];
  double T[12];
  block_procrustes(src_corr, ref_corr, scores, nullptr, x0, x1, red, T);
  if (threadIdx.x < 12) {
    Tf[threadIdx.x] = static_cast<float>(T[threadIdx.x]);
    w.chunk_T[12 * chunk + threadIdx.x] = Tf[threadIdx.x];
  }
  if (threadIdx.x == 0) cnt_sh = 0;
  __syncthreads();
  const int C = w.ver_s ? w.meta[3] : w.meta[0];  // (correspondence_limit: fitted on the patch, scored on the verification set)
  const float* vs = w.ver_s ? w.ver_src : src_corr;
  const float* vr = w.ver_s ? w.ver_ref : ref_corr;
  int c = 0;
  for (int i = threadIdx.x; i < C; i += blockDim.x) c += is_inlier(Tf, vs, vr, i, radius) ? 1 : 0;
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt_sh, c);
  __syncthreads();
  if (threadIdx.x == 0) w.chunk_inliers[chunk] = cnt_sh;
}
// single block: pick the hypothesis, refine globally
constexpr int kRefineStage = 4608;  // correspondences staged in LDS: 4608 * 29 B = 131 KB
__device__ __forceinline__ void lgr_refine_kernel_body(const dim3 blockIdx, const dim3 gridDim, const float* ref_corr, const float* src_corr,
                                                          const float* scores, float radius, int steps,
                                                          LgrBuffers w, unsigned char* gate, float* out_T,
                                                          int32_t* counts) {
  (void)blockIdx; (void)gridDim;
  __shared__ double red[9 * 16];
  __shared__ float Tf[12];
  extern __shared__ float stage[];
  const int C = w.ver_s ? w.meta[3] : w.meta[0], chunks = w.meta[1];  // (correspondence_limit: the arguments are the verification set)
  int best_out = w.meta[2];  // (the layout kernel's value when no patch reaches the threshold)
  // The refinement makes 4 passes over the correspondences per step; one workgroup, so every pass is a chain of
  // dependent L2 round trips.  Up to kRefineStage correspondences are copied into LDS once (7 words each + the gate).
  if (C <= kRefineStage) {
    float* ls = stage;
    float* lr = ls + 3 * C;
    float* lw = lr + 3 * C;
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) {
      ls[i] = src_corr[i];
      lr[i] = ref_corr[i];
    }
    for (int i = threadIdx.x; i < C; i += blockDim.x) lw[i] = scores[i];
    src_corr = ls; ref_corr = lr; scores = lw;
    gate = reinterpret_cast<unsigned char*>(lw + C);
    __syncthreads();
  }
  double T[12];
  if (chunks > 0) {
    // first maximum of the inlier counts (torch.argmax): block-wide max of (count, -index) packed in 64 bits
    __shared__ unsigned long long s_best[4];
    unsigned long long mine = 0;
    for (int k = threadIdx.x; k < chunks; k += blockDim.x)
      mine = max(mine, (static_cast<unsigned long long>(static_cast<unsigned>(w.chunk_inliers[k])) << 32) |
                           static_cast<unsigned>(0x7fffffff - k));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine = max(mine, static_cast<unsigned long long>(__shfl_xor(mine, o, 64)));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = mine;
    __syncthreads();
    const unsigned long long all = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
    const int best = 0x7fffffff - static_cast<int>(all & 0xffffffffull);
    if (threadIdx.x == 0) w.meta[2] = best;
    best_out = best;
    if (threadIdx.x < 12) Tf[threadIdx.x] = w.chunk_T[12 * best + threadIdx.x];
  } else {  // degenerate: no patch reaches the threshold -> start from all correspondences (:189-194)
    block_procrustes(src_corr, ref_corr, scores, nullptr, 0, C, red, T);
    if (threadIdx.x < 12) Tf[threadIdx.x] = static_cast<float>(T[threadIdx.x]);
  }
  __syncthreads();
  double basis[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};  // eigenvector frame carried from step to step
  for (int step = 0; step < steps; ++step) {
    for (int i = threadIdx.x; i < C; i += blockDim.x) gate[i] = is_inlier(Tf, src_corr, ref_corr, i, radius) ? 1 : 0;
    __syncthreads();
    block_procrustes(src_corr, ref_corr, scores, gate, 0, C, red, T, basis);
    __syncthreads();
    if (threadIdx.x < 12) Tf[threadIdx.x] = static_cast<float>(T[threadIdx.x]);
    __syncthreads();
  }
  if (threadIdx.x < 16) {
    const int r = threadIdx.x / 4, c = threadIdx.x % 4;
    out_T[threadIdx.x] = r < 3 ? Tf[4 * r + c] : (c == 3 ? 1.f : 0.f);
  }
  if (threadIdx.x == 0) {  // {n_correspondences, n_hypotheses, best_hypothesis} for the caller (no separate copy launch)
    counts[0] = w.meta[0];
    counts[1] = chunks;
    counts[2] = best_out;
  }
}
}  // namespace

namespace {

// matches a patch can hold with top-k: k per real row + k per real column, and never more than the block (the default path keeps
// kPerPatch = 2 * 128 whatever the side)
int64_t lgr_options_stride(int64_t side, int k) {
  return std::min<int64_t>(2 * static_cast<int64_t>(k) * side, side * side);
}

// The workspace of one call: `stride` matches per patch, verification arrays for `ver` correspondences (0: no limit).
unsigned char* lgr_take(rdm::Arena& ar, size_t b, size_t stride, size_t ver, LgrBuffers& w) {
  w.patch_count = ar.take<int32_t>(b);
  w.patch_offset = ar.take<int32_t>(b);
  w.chunk_patch = ar.take<int32_t>(b);
  w.meta = ar.take<int32_t>(4);
  w.local_i = ar.take<int32_t>(b * stride);
  w.local_j = ar.take<int32_t>(b * stride);
  w.local_s = ar.take<float>(b * stride);
  w.chunk_T = ar.take<float>(b * 12);
  w.chunk_inliers = ar.take<int32_t>(b);
  unsigned char* gate = ar.take<unsigned char>(b * stride);
  w.stride = static_cast<int>(stride);
  w.ver_ref = w.ver_src = w.ver_s = nullptr;
  if (ver > 0) {
    w.ver_ref = ar.take<float>(3 * ver);
    w.ver_src = ar.take<float>(3 * ver);
    w.ver_s = ar.take<float>(ver);
  }
  return gate;
}

const char* lgr_options_error(const rdm_fine_matching_options* o, int64_t side) {
  if (!o) return "options is null";
  if (o->topk < 1 || o->topk > side + (o->use_dustbin ? 1 : 0)) return "topk must be in [1, side] ([1, side + 1] with use_dustbin)";
  if (!(o->confidence_threshold >= 0.f)) return "confidence_threshold must be >= 0";
  if (o->correspondence_limit < 0) return "correspondence_limit must be 0 (none) or >= 1";
  return nullptr;
}

size_t lgr_ver_rows(int64_t batch, int64_t stride, const rdm_fine_matching_options* o) {
  return o && o->correspondence_limit > 0 ? static_cast<size_t>(std::min<int64_t>(o->correspondence_limit, batch * stride)) : 0;
}

// opt == nullptr: the shipped configuration with its own extraction kernel (rdm_lgr)
int lgr_run(const char* who, const float* log_scores, int64_t score_dim, const float* ref_knn_points, const float* src_knn_points,
            const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, const float* global_scores, int64_t batch, int64_t side,
            float acceptance_radius, int correspondence_threshold, int num_refinement_steps, const rdm_fine_matching_options* opt,
            float* ref_corr, float* src_corr, float* corr_scores, float* transform, int32_t* counts, void* ws, size_t ws_bytes,
            void* stream) {
  using namespace rdm;
  RDM_REQUIRE(log_scores && ref_knn_points && src_knn_points && ref_knn_masks && src_knn_masks && ref_corr &&
                  src_corr && corr_scores && transform && counts, "%s: null pointer", who);
  RDM_REQUIRE(batch > 0 && side > 0 && side <= kSide, "%s: bad sizes (batch=%lld side=%lld)", who,
              (long long)batch, (long long)side);
  const size_t b = static_cast<size_t>(batch);
  const size_t stride = opt ? static_cast<size_t>(lgr_options_stride(side, opt->topk)) : kPerPatch;
  Arena ar(ws, ws_bytes);
  LgrBuffers w;
  unsigned char* gate = lgr_take(ar, b, stride, lgr_ver_rows(batch, static_cast<int64_t>(stride), opt), w);
  if (!ar.ok) {
    set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int S = static_cast<int>(side), B = static_cast<int>(batch);
  const size_t lds = sizeof(float) * (S + 1) * ((S + 1) | 1);
  if (opt) {
    const LgrSelect sel{opt->topk, opt->mutual != 0, opt->use_dustbin != 0, opt->use_global_score != 0, opt->confidence_threshold};
    ::rdm::launch<lgr_extract_topk_kernel_body, 256>(dim3(B), lds, st, log_scores, static_cast<int>(score_dim), S,
                       ref_knn_masks, src_knn_masks, global_scores, sel, w);
  } else {
    ::rdm::launch<lgr_extract_kernel_body, 256>(dim3(B), lds, st, log_scores, S, ref_knn_masks, src_knn_masks, w);
  }
  ::rdm::launch<lgr_layout_kernel_body, 64>(dim3(1), 0, st, B, correspondence_threshold, w);
  ::rdm::launch<lgr_gather_kernel_body, 64>(dim3(B), 0, st, ref_knn_points, src_knn_points, S, w, ref_corr,
                     src_corr, corr_scores);
  if (w.ver_s)
    ::rdm::launch<lgr_limit_kernel_body, kLimitThreads>(dim3(1), 0, st, ref_corr, src_corr, corr_scores,
                       opt->correspondence_limit, w);
  ::rdm::launch<lgr_local_kernel_body, 256>(dim3(B), 0, st, ref_corr, src_corr, corr_scores, acceptance_radius, w);
  // (with a limit the refinement runs on the verification set; counts[0] stays the number of ALL correspondences)
  ::rdm::launch<lgr_refine_kernel_body, 256>(dim3(1), kRefineStage * 29 + 64, st, w.ver_s ? w.ver_ref : ref_corr,
                     w.ver_s ? w.ver_src : src_corr, w.ver_s ? w.ver_s : corr_scores, acceptance_radius, num_refinement_steps, w, gate,
                     transform, counts);
  return launch_status("lgr kernels");
}

}  // namespace

extern "C" size_t rdm_lgr_workspace_bytes(int64_t batch) {
  rdm::Arena a(nullptr, 0);
  LgrBuffers w;
  lgr_take(a, static_cast<size_t>(batch > 0 ? batch : 1), kPerPatch, 0, w);
  return a.off;
}

// log_scores [batch, side+1, side+1] (Sinkhorn output), knn points [batch, side, 3], masks [batch, side].
// Outputs (capacity batch*2*side rows): ref_corr/src_corr [.,3], corr_scores [.], transform [16],
// counts [3] = {n_correspondences, n_hypotheses, best_hypothesis} (device int32).
extern "C" int rdm_lgr(const float* log_scores, const float* ref_knn_points, const float* src_knn_points,
                       const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, int64_t batch, int64_t side,
                       float acceptance_radius, int correspondence_threshold, int num_refinement_steps,
                       float* ref_corr, float* src_corr, float* corr_scores, float* transform, int32_t* counts,
                       void* ws, size_t ws_bytes, void* stream) {
  return lgr_run("rdm_lgr", log_scores, side + 1, ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, nullptr, batch, side,
                 acceptance_radius, correspondence_threshold, num_refinement_steps, nullptr, ref_corr, src_corr, corr_scores, transform,
                 counts, ws, ws_bytes, stream);
}

extern "C" int64_t rdm_lgr_options_capacity(int64_t batch, int64_t side, const rdm_fine_matching_options* options) {
  if (batch <= 0 || side <= 0 || side > kSide || lgr_options_error(options, side)) return 0;
  return batch * lgr_options_stride(side, options->topk);
}

extern "C" size_t rdm_lgr_options_workspace_bytes(int64_t batch, int64_t side, const rdm_fine_matching_options* options) {
  if (side <= 0 || side > kSide || lgr_options_error(options, side)) return 0;
  rdm::Arena a(nullptr, 0);
  LgrBuffers w;
  const int64_t b = batch > 0 ? batch : 1, stride = lgr_options_stride(side, options->topk);
  lgr_take(a, static_cast<size_t>(b), static_cast<size_t>(stride), lgr_ver_rows(b, stride, options), w);
  return a.off;
}

// rdm_lgr with every key of cfg.fine_matching.  log_scores [batch, score_dim, score_dim]: score_dim = side + 1 (the Sinkhorn
// output; without use_dustbin only its [side, side] block is read) or, without use_dustbin, side (the block alone).
// Outputs have capacity rdm_lgr_options_capacity(batch, side, options) rows.
extern "C" int rdm_lgr_options(const float* log_scores, int64_t score_dim, const float* ref_knn_points, const float* src_knn_points,
                               const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, const float* global_scores, int64_t batch,
                               int64_t side, float acceptance_radius, int correspondence_threshold, int num_refinement_steps,
                               const rdm_fine_matching_options* options, float* ref_corr, float* src_corr, float* corr_scores,
                               float* transform, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(side > 0 && side <= kSide, "rdm_lgr_options: bad sizes (side=%lld)", (long long)side);
  const char* bad = lgr_options_error(options, side);
  RDM_REQUIRE(bad == nullptr, "rdm_lgr_options: %s", bad ? bad : "");
  RDM_REQUIRE(score_dim == side + 1 || (score_dim == side && !options->use_dustbin),
              "rdm_lgr_options: score_dim %lld is neither side + 1 nor (without use_dustbin) side = %lld", (long long)score_dim,
              (long long)side);
  RDM_REQUIRE(global_scores || !options->use_global_score, "rdm_lgr_options: use_global_score without global_scores");
  return lgr_run("rdm_lgr_options", log_scores, score_dim, ref_knn_points, src_knn_points, ref_knn_masks, src_knn_masks, global_scores,
                 batch, side, acceptance_radius, correspondence_threshold, num_refinement_steps, options, ref_corr, src_corr,
                 corr_scores, transform, counts, ws, ws_bytes, stream);
}
