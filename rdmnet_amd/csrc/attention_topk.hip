// Top-k ("dynamic") self-attention of the second 3DRoFormer (cfg.thdroformer.k2).
//
// Reference: rdmnet/thdroformer/thdroformer.py:20-40 (dynamic_attention with k != None), :132-135 (the self layer passes
// k[layer]), :204-251 (k reaches the 'self' blocks only).  Each query row keeps its `keep` largest scores q.k / sqrt(32);
// softmax runs over the kept scores alone and the other keys get probability 0.  Ties at the boundary (torch.topk leaves the
// choice open): among keys whose score equals the keep-th largest, the lowest key indices are kept.
//
// One workgroup = 16 queries of one head (d = 32), as in attention.hip: its four wavefronts split the key tiles (tile % 4 ==
// wave) and the score tile S^T[key][query] comes from the same v_mfma_f32_16x16x4_f32 sequence and the same division by
// sqrt(d) as the dense kernel.  A tile's scores live in the lane that formed them: lane (x, g) holds keys 4g .. 4g+3 of query x.
//   1. Scores: every tile is formed once and kept in LDS as one float4 per lane (conflict-free 16-byte reads), 1 KiB per 16
//      keys, when the segment has at most kStageKeys keys; above that every pass below forms the tile again -- the same MFMA
//      sequence on the same operands, so every pass reads the same fp32 scores.  The first pass also takes the row maximum.
//   2. Select: on order-preserving uint32 keys of the scores (-0 read as +0), the keep-th largest key T is found bit by bit
//      from the top, each bit one counting pass (per-lane counts, a cross-lane sum, a cross-wave sum through LDS).  Then, if
//      more keys equal T than the rank left over, the last kept index J among them is found the same way on the key index.
//      Kept: key > T, or key == T and index <= J.
//   3. Softmax over the kept set (its maximum is the row maximum) and P V on the MFMA with P = 0 outside the set; the four
//      wavefronts' partial sums are added in wave order.
// keep == 0 writes zero rows (the reference's empty topk scatters nothing); keep >= nk skips the select (every key kept).
#include "../../include/rdmnet_hip.h"
#include "common.h"
#include "lockstep.h"

namespace {

using namespace rdm;

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kHeadDim = 32;
constexpr int kStageKeys = 2048;  // rows up to this many keys keep their score tile in LDS (64 B per key: 128 KiB)
constexpr size_t kPartialBytes = 4 * 16 * (kHeadDim + 1) * sizeof(float);  // the four waves' partial outputs (8448 B)
static_assert(kPartialBytes % 16 == 0, "the score tile after the partials must stay 16-byte aligned");

struct TopkArgs {
  const float* q;
  const float* k;
  const float* v;
  float* out;
  int nq, nk, keep, heads;
  int ldq, ldk, ldv, ldo;
  float inv_scale;  // sqrt(d)
  // optional second, independent segment (the second cloud of a self-attention pair): workgroups blockIdx.x >= seg0_blocks take
  // rows starting at `row1`, nq1 / nk1 rows, keep1 kept keys; seg0_blocks = 0: none
  int seg0_blocks, row1, nq1, nk1, keep1;
};

__device__ __forceinline__ void attention_topk_body(const dim3 blockIdx, const dim3 gridDim, TopkArgs a_in) {
  (void)gridDim;
  TopkArgs a = a_in;
  int bx = blockIdx.x;
  if (a.seg0_blocks > 0 && bx >= a.seg0_blocks) {  // block-uniform: the second cloud's rows
    bx -= a.seg0_blocks;
    a.q += static_cast<int64_t>(a.row1) * a.ldq;
    a.k += static_cast<int64_t>(a.row1) * a.ldk;
    a.v += static_cast<int64_t>(a.row1) * a.ldv;
    a.out += static_cast<int64_t>(a.row1) * a.ldo;
    a.nq = a.nq1;
    a.nk = a.nk1;
    a.keep = a.keep1;
  }
  // dynamic LDS: the partial outputs, then (stage) the score tile [tile][lane].  Static LDS stays under 4 KB, so the 156 KB
  // dynamic-LDS attribute lockstep.h sets on a grouped instance is valid for this kernel too.
  extern __shared__ f32x4 s_dyn[];
  float (*s_o)[16][kHeadDim + 1] = reinterpret_cast<float (*)[16][kHeadDim + 1]>(s_dyn);
  f32x4* s_tile = s_dyn + kPartialBytes / sizeof(f32x4);
  __shared__ int s_cnt[4][16];
  __shared__ float s_max[4][16], s_l[4][16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q0 = bx * 16;
  const int head = blockIdx.y;
  const int g = lane >> 4, x = lane & 15;
  const int hoff = head * kHeadDim;
  const int nk = a.nk;
  const int keep = min(a.keep, nk);
  const bool stage = nk <= kStageKeys;  // block-uniform; the launch reserved ceil(nk / 16) KiB for every segment that stages

  if (keep <= 0) {  // block-uniform: zero rows (thread t writes query t >> 4, features 2 * (t & 15), +1)
    const int qi = q0 + (threadIdx.x >> 4), dd = 2 * (threadIdx.x & 15);
    if (qi < a.nq) *reinterpret_cast<float2*>(a.out + static_cast<int64_t>(qi) * a.ldo + hoff + dd) = make_float2(0.f, 0.f);
    return;
  }

  // Q fragment: query q0+x, features 8g .. 8g+7 of this head (contraction index = 8*kappa + step), as in attention.hip
  float qf[8];
  {
    const int qi = min(q0 + x, a.nq - 1);
    const float4* p = reinterpret_cast<const float4*>(a.q + static_cast<int64_t>(qi) * a.ldq + hoff + 8 * g);
    const float4 u = p[0], w = p[1];
    qf[0] = u.x; qf[1] = u.y; qf[2] = u.z; qf[3] = u.w;
    qf[4] = w.x; qf[5] = w.y; qf[6] = w.z; qf[7] = w.w;
  }
  // S^T[key k0+4g+r][query x] of the tile at k0 (keys past nk: unspecified, callers test the index)
  auto form = [&](int k0) -> f32x4 {
    const int ki = min(k0 + x, nk - 1);
    const float4* p = reinterpret_cast<const float4*>(a.k + static_cast<int64_t>(ki) * a.ldk + hoff + 8 * g);
    const float4 u = p[0], w = p[1];
    const float kf[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t], qf[t], s, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = s[r] / a.inv_scale;
    return s;
  };
  auto scores = [&](int k0) -> f32x4 { return stage ? s_tile[(k0 >> 4) * 64 + lane] : form(k0); };
  // the 16 queries' totals over every key of a per-lane count; every thread returns its query x's total
  auto total = [&](int c) -> int {
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    __syncthreads();  // (the previous pass's readers are done with s_cnt)
    if (g == 0) s_cnt[wave][x] = c;
    __syncthreads();
    return s_cnt[0][x] + s_cnt[1][x] + s_cnt[2][x] + s_cnt[3][x];
  };

  // ---- 1. scores (staged in LDS when they fit) and the row maximum
  float mx = -INFINITY;
  for (int k0 = wave * 16; k0 < nk; k0 += 64) {
    const f32x4 s = form(k0);
    if (stage) s_tile[(k0 >> 4) * 64 + lane] = s;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (k0 + 4 * g + r < nk) mx = fmaxf(mx, s[r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  if (g == 0) s_max[wave][x] = mx;
  __syncthreads();  // (also publishes the staged tile)
  mx = fmaxf(fmaxf(s_max[0][x], s_max[1][x]), fmaxf(s_max[2][x], s_max[3][x]));

  // ---- 2. select: the keep-th largest order key T of query x, then the last kept index J among the keys equal to T
  uint32_t T = 0;
  int J = nk;  // keep >= nk: T = 0 and J = nk keep every key
  if (keep < nk) {
    int need = keep;  // rank of the wanted key among the keys that match the prefix found so far
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t hi = ~((1u << bit) - 1u), cand = T | (1u << bit);
      int c = 0;
      for (int k0 = wave * 16; k0 < nk; k0 += 64) {
        const f32x4 s = scores(k0);
#pragma unroll
        for (int r = 0; r < 4; ++r) c += (k0 + 4 * g + r < nk && (order_key(s[r] + 0.0f) & hi) == cand) ? 1 : 0;
      }
      c = total(c);
      if (c >= need) T = cand;
      else need -= c;
    }
    // `need` is now the number of keys equal to T that are kept, by lowest index
    int c = 0;
    for (int k0 = wave * 16; k0 < nk; k0 += 64) {
      const f32x4 s = scores(k0);
#pragma unroll
      for (int r = 0; r < 4; ++r) c += (k0 + 4 * g + r < nk && order_key(s[r] + 0.0f) == T) ? 1 : 0;
    }
    const int n_eq = total(c);
    if (__syncthreads_or(need < n_eq)) {  // some query cuts its ties: find the need-th of them in index order
      int lim = 0;  // J = the smallest index with #{j <= J : key_j == T} >= need, bit by bit from the top
      int rem = need;
      const int bits = 32 - __clz(nk - 1);
      for (int bit = bits - 1; bit >= 0; --bit) {
        const int cand = lim | (1 << bit);  // count the equal keys in [lim, cand): is the need-th one below cand?
        int cc = 0;
        for (int k0 = wave * 16; k0 < nk; k0 += 64) {
          const f32x4 s = scores(k0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = k0 + 4 * g + r;
            cc += (j < nk && j >= lim && j < cand && order_key(s[r] + 0.0f) == T) ? 1 : 0;
          }
        }
        cc = total(cc);
        if (cc < rem) {
          rem -= cc;
          lim = cand;
        }
      }
      if (need < n_eq) J = lim;  // (the need-th equal key sits at index lim)
    }
  }

  // ---- 3. softmax over the kept set and O = P V (P = 0 outside it)
  float lsum = 0.f;
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};  // O[query 4g+r][d = 2x + t]
  for (int k0 = wave * 16; k0 < nk; k0 += 64) {
    const f32x4 s = scores(k0);
    float2 vv[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int kj = min(k0 + 4 * g + st, nk - 1);
      vv[st] = *reinterpret_cast<const float2*>(a.v + static_cast<int64_t>(kj) * a.ldv + hoff + 2 * x);
    }
    f32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = k0 + 4 * g + r;
      const uint32_t key = order_key(s[r] + 0.0f);
      const bool kept = j < nk && (key > T || (key == T && j <= J));
      p[r] = kept ? expf(s[r] - mx) : 0.f;
      lsum += p[r];
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[st], vv[st].x, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[st], vv[st].y, o1, 0, 0, 0);
    }
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  if (g == 0) s_l[wave][x] = lsum;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s_o[wave][4 * g + r][2 * x] = o0[r];
    s_o[wave][4 * g + r][2 * x + 1] = o1[r];
  }
  __syncthreads();
  {
    const int qq = threadIdx.x >> 4, dd = 2 * (threadIdx.x & 15);
    const int qi = q0 + qq;
    float lt = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      lt += s_l[w][qq];
      a0 += s_o[w][qq][dd];
      a1 += s_o[w][qq][dd + 1];
    }
    if (qi < a.nq)
      *reinterpret_cast<float2*>(a.out + static_cast<int64_t>(qi) * a.ldo + hoff + dd) = make_float2(a0 / lt, a1 / lt);
  }
}

// Fills the segment-independent fields, sizes the staged tile for the largest segment that stages, and launches.
int topk_launch(TopkArgs a, int64_t blocks, int heads, hipStream_t stream) {
  a.heads = heads;
  a.inv_scale = sqrtf(static_cast<float>(kHeadDim));
  int64_t staged = 0;
  for (const int64_t n : {int64_t(a.nk), int64_t(a.seg0_blocks > 0 ? a.nk1 : 0)})
    if (n <= kStageKeys && n > staged) staged = n;
  const size_t lds = kPartialBytes + static_cast<size_t>(ceil_div<int64_t>(staged, 16)) * 64 * sizeof(f32x4);
  const dim3 grid(static_cast<unsigned>(blocks), heads);
  launch<attention_topk_body, 256>(grid, lds, stream, a);
  return launch_status("attention_topk_kernel");
}

int check_common(const float* q, const float* k, const float* v, float* out, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                 int heads, int head_dim, const char* who) {
  RDM_REQUIRE(q && k && v && out, "%s: null pointer", who);
  RDM_REQUIRE(head_dim == kHeadDim, "%s: head_dim must be %d", who, kHeadDim);
  RDM_REQUIRE(heads > 0, "%s: bad sizes", who);
  RDM_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 2 == 0 && ldo % 2 == 0, "%s: strides must be padded", who);
  return RDM_OK;
}

}  // namespace

extern "C" int64_t rdm_topk_count(int64_t n, double frac) {
  // Python's int(n * f): the IEEE double product, truncated toward zero (int(100 * 0.57) == 56)
  return static_cast<int64_t>(static_cast<double>(n) * frac);
}

extern "C" int rdm_attention_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                                  int64_t ldo, int64_t n_q, int64_t n_k, int64_t keep, int heads, int head_dim, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(n_q >= 0 && n_k >= 0 && heads > 0 && keep >= 0 && keep <= n_k && n_k < (int64_t(1) << 30),
              "rdm_attention_topk: bad sizes");
  if (n_q == 0) return RDM_OK;  // (torch hands zero-row tensors over as null pointers)
  if (check_common(q, n_k ? k : q, n_k ? v : q, out, ldq, ldk, ldv, ldo, heads, head_dim, "rdm_attention_topk") != RDM_OK)
    return RDM_ERR_ARG;
  TopkArgs a;
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.nq = static_cast<int>(n_q); a.nk = static_cast<int>(n_k); a.keep = static_cast<int>(keep);
  a.ldq = static_cast<int>(ldq); a.ldk = static_cast<int>(ldk); a.ldv = static_cast<int>(ldv); a.ldo = static_cast<int>(ldo);
  a.seg0_blocks = 0; a.row1 = 0; a.nq1 = 0; a.nk1 = 0; a.keep1 = 0;
  return topk_launch(a, ceil_div<int64_t>(n_q, 16), heads, static_cast<hipStream_t>(stream));
}

// Both stacked clouds in one launch: rows [0, n0) attend to rows [0, n0) keeping keep0 keys, rows [n0, n0 + n1) to rows
// [n0, n0 + n1) keeping keep1; the same bits as two rdm_attention_topk calls.
extern "C" int rdm_attention_self_pair_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                            float* out, int64_t ldo, int64_t n0, int64_t n1, int64_t keep0, int64_t keep1, int heads,
                                            int head_dim, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(n0 >= 0 && n1 >= 0 && heads > 0 && n0 + n1 < (int64_t(1) << 30) && keep0 >= 0 && keep0 <= n0 && keep1 >= 0 &&
                  keep1 <= n1,
              "rdm_attention_self_pair_topk: bad sizes");
  if (n0 + n1 == 0) return RDM_OK;
  if (check_common(q, k, v, out, ldq, ldk, ldv, ldo, heads, head_dim, "rdm_attention_self_pair_topk") != RDM_OK) return RDM_ERR_ARG;
  if (n0 == 0 || n1 == 0) {  // one cloud is empty: the plain launch on the other (it starts at row 0 either way)
    const int64_t n = n0 + n1;
    return rdm_attention_topk(q, ldq, k, ldk, v, ldv, out, ldo, n, n, n0 ? keep0 : keep1, heads, head_dim, stream);
  }
  TopkArgs a;
  a.q = q; a.k = k; a.v = v; a.out = out;
  a.nq = static_cast<int>(n0); a.nk = static_cast<int>(n0); a.keep = static_cast<int>(keep0);
  a.ldq = static_cast<int>(ldq); a.ldk = static_cast<int>(ldk); a.ldv = static_cast<int>(ldv); a.ldo = static_cast<int>(ldo);
  a.seg0_blocks = static_cast<int>(ceil_div<int64_t>(n0, 16));
  a.row1 = static_cast<int>(n0); a.nq1 = static_cast<int>(n1); a.nk1 = static_cast<int>(n1); a.keep1 = static_cast<int>(keep1);
  return topk_launch(a, a.seg0_blocks + ceil_div<int64_t>(n1, 16), heads, static_cast<hipStream_t>(stream));
}
