// DESIGN.md §7 -- the offline evaluator: what experiments/eval.py:100-239 computes per saved pair file, for a batch of P
// pairs per call.  Four kernels, whatever P is (method RANSAC adds rdm_ransac_correspondences' three per pair):
//   eval_select_kernel      one workgroup per pair   --num_corr: the L best-scored rows, radix select as lgr_limit_kernel
//   eval_procrustes_kernel  one workgroup per pair   method svd: weighted Procrustes, float64 sums, Horn's solver
//   eval_fine_kernel        (row tiles, pairs)       residuals, inlier counts and the exact nearest-neighbour search of
//                                                    `overlap` (moved src rows staged in LDS), one partial per tile
//   eval_finish_kernel      one workgroup per pair   the tiles' partials in tile order, the coarse precision (cell maps
//                                                    in LDS), the registration error, the record
// No atomics anywhere: counts go through ballots / wave sums and a fixed-order LDS pass, float64 sums likewise, so a
// pair's record is the same alone and inside any batch.
#include "../../include/rdmnet_hip.h"
#include "common.h"
#include "procrustes.h"

#pragma clang fp contract(off)

namespace {
using namespace rdm;

constexpr int kSelectThreads = 1024;
constexpr int kFineThreads = 256;    // ref rows per tile, one per thread
constexpr int kSrcTile = 1024;       // moved src rows staged per round (float4: 16 KB)
constexpr int kCellChunk = 28 * 1024;  // cells per round of the coarse precision: two byte maps, 56 KB of LDS
constexpr int kFinishThreads = 256;

struct FinePartial {
  double residual_sum;
  int32_t inliers[3];  // acceptance radius, 0.3, 0.1
  int32_t overlap;
};

// rows of pair p that are evaluated: min(C, L)
__device__ __forceinline__ int selected_rows(const int64_t* corr_offsets, int p, int limit) {
  const int c = static_cast<int>(corr_offsets[p + 1] - corr_offsets[p]);
  return (limit > 0 && c > limit) ? limit : c;
}

// ------------------------------------------------------------------------------------------------------------ select
// eval.py:121-125 per pair segment.  C > L: the first L rows in the order (score descending, row ascending), written in row
// order to the head of the pair's segment of sel_* (same offsets as the inputs).  An 8-bit radix select on the keys finds the
// L-th score (4 histogram passes; the histogram is filled from per-wave ballots of each digit's candidates -- no atomics),
// then one ordered pass keeps what is above it and the first `need` rows equal to it.  C <= L: every row, copied.
__global__ __launch_bounds__(kSelectThreads) void eval_select_kernel(const int64_t* __restrict__ corr_offsets,
                                                                     const float* __restrict__ ref_corr,
                                                                     const float* __restrict__ src_corr,
                                                                     const float* __restrict__ scores, int limit,
                                                                     float* __restrict__ sel_ref, float* __restrict__ sel_src,
                                                                     float* __restrict__ sel_scores) {
  constexpr int kWaves = kSelectThreads / 64;
  __shared__ int hist[kWaves][256];  // per-wave digit counts: each wave owns its row, plain stores
  __shared__ int total[256];
  __shared__ unsigned s_prefix;
  __shared__ int s_need;
  __shared__ int wsum[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t begin = corr_offsets[blockIdx.x];
  const int C = static_cast<int>(corr_offsets[blockIdx.x + 1] - begin);
  const float* sc = scores + begin;
  const bool all = C <= limit;
  unsigned prefix = 0;
  int need = limit;  // rank of the L-th score among the keys that share `prefix` above the current digit
  if (!all) {
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int d = lane; d < 256; d += 64) hist[wave][d] = 0;
      __syncthreads();
      const unsigned above = shift == 24 ? 0u : ~0u << (shift + 8);
      for (int i0 = wave * 64; i0 < C; i0 += kSelectThreads) {
        const int i = i0 + lane;
        unsigned digit = 256u;  // no candidate
        if (i < C) {
          const unsigned key = order_key(sc[i]);
          if ((key & above) == prefix) digit = (key >> shift) & 255u;
        }
        // lanes with the same digit: the lowest of them adds the group's size to the wave's own row
        unsigned long long pending = __builtin_amdgcn_ballot_w64(digit < 256u);
        while (pending) {
          const int leader = __builtin_ctzll(pending);
          const unsigned d = static_cast<unsigned>(__shfl(static_cast<int>(digit), leader, 64));
          const unsigned long long same = __builtin_amdgcn_ballot_w64(digit == d);
          if (lane == leader) hist[wave][d] += __popcll(same);
          pending &= ~same;
        }
      }
      __syncthreads();
      if (tid < 256) {
        int t = 0;
        for (int v = 0; v < kWaves; ++v) t += hist[v][tid];
        total[tid] = t;
      }
      __syncthreads();
      if (wave == 0) {  // lane l owns digits 255 - 4l .. 252 - 4l: the digit that holds the need-th key from the top
        int h[4], local = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          h[u] = total[255 - 4 * lane - u];
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
  int base_g = 0, base_e = 0;  // rows above / equal to the L-th score before this tile (identical in all threads)
  for (int i0 = 0; i0 < C; i0 += kSelectThreads) {
    const int i = i0 + tid;
    bool g = false, e = false;
    if (i < C) {
      const unsigned key = order_key(sc[i]);
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
    for (int v = 0; v < kWaves; ++v) {
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
      const int64_t dst = begin + base_g + og + (eq_before < need ? eq_before : need);  // < begin + min(C, L)
      const int64_t row = begin + i;
      for (int d = 0; d < 3; ++d) {
        sel_ref[3 * dst + d] = ref_corr[3 * row + d];
        sel_src[3 * dst + d] = src_corr[3 * row + d];
      }
      sel_scores[dst] = sc[i];
    }
    base_g += tg;
    base_e += te;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ block reductions
// Sum over the workgroup in a fixed order: lanes by butterfly, waves in ascending order.  Result in every thread.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* scratch /* THREADS / 64 */) {
  v = wave_sum(v);
  __syncthreads();  // (scratch may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) t += scratch[w];
  return t;
}
template <int THREADS>
__device__ __forceinline__ int block_sum_i(int v, int* scratch) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) t += scratch[w];
  return t;
}

// ------------------------------------------------------------------------------------------------------- procrustes
// weighted_procrustes(src, ref, scores) (procrustes.py:6-73, weight_thresh 0, eps 1e-5): w = s / (sum s + eps),
// centroids sum w p (not renormalised, as the reference), H = sum w (src - cs)(ref - cr)^T, R = Kabsch(H), t = cr - R cs.
__global__ __launch_bounds__(256) void eval_procrustes_kernel(const int64_t* __restrict__ corr_offsets, int limit,
                                                              const float* __restrict__ ref, const float* __restrict__ src,
                                                              const float* __restrict__ scores, float* __restrict__ est) {
  __shared__ double scratch[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t begin = corr_offsets[p];
  const int n = selected_rows(corr_offsets, p, limit);
  double sw = 0.0;
  for (int i = tid; i < n; i += 256) {
    const float s = scores[begin + i];
    sw += s < 0.f ? 0.0 : static_cast<double>(s);
  }
  const double denom = block_sum<256>(sw, scratch) + 1e-5;
  double c[6] = {0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += 256) {
    const float s = scores[begin + i];
    const double w = (s < 0.f ? 0.0 : static_cast<double>(s)) / denom;
    for (int d = 0; d < 3; ++d) {
      c[d] += w * src[3 * (begin + i) + d];
      c[3 + d] += w * ref[3 * (begin + i) + d];
    }
  }
  for (int d = 0; d < 6; ++d) c[d] = block_sum<256>(c[d], scratch);
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += 256) {
    const float s = scores[begin + i];
    const double w = (s < 0.f ? 0.0 : static_cast<double>(s)) / denom;
    double a[3], b[3];
    for (int d = 0; d < 3; ++d) {
      a[d] = src[3 * (begin + i) + d] - c[d];
      b[d] = w * (ref[3 * (begin + i) + d] - c[3 + d]);
    }
    for (int x = 0; x < 3; ++x)
      for (int y = 0; y < 3; ++y) H[3 * x + y] += a[x] * b[y];
  }
  for (int k = 0; k < 9; ++k) H[k] = block_sum<256>(H[k], scratch);
  if (tid == 0) {
    double R[9];
    kabsch_rotation(H, R);
    float* T = est + 16ll * p;
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) T[4 * a + b] = static_cast<float>(R[3 * a + b]);
      T[4 * a + 3] = static_cast<float>(c[3 + a] - (R[3 * a] * c[0] + R[3 * a + 1] * c[1] + R[3 * a + 2] * c[2]));
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
  }
}

// ------------------------------------------------------------------------------------------------------------- fine
// apply_transform in fp32 (pointcloud.py: p R^T + t): the k = 3 product as the sgemm behind np.matmul forms it, then + t
__device__ __forceinline__ float3 move_point(const float* __restrict__ T, float x, float y, float z) {
  float3 r;
  r.x = fmaf(z, T[2], fmaf(y, T[1], x * T[0])) + T[3];
  r.y = fmaf(z, T[6], fmaf(y, T[5], x * T[4])) + T[7];
  r.z = fmaf(z, T[10], fmaf(y, T[9], x * T[8])) + T[11];
  return r;
}

// Tile t of pair p: ref rows 256 t .. 256 t + 255 of the selected rows, one per thread.  Own correspondence: the fp32
// residual of registration.py:175-188.  Overlap: the nearest moved src row by exact search over LDS tiles (the coordinate
// differences of two fp32 numbers are exact at these ranges; d2 in fp32, compared as sqrt in float64).
__global__ __launch_bounds__(kFineThreads) void eval_fine_kernel(const int64_t* __restrict__ corr_offsets, int limit,
                                                                 const float* __restrict__ ref, const float* __restrict__ src,
                                                                 const float* __restrict__ gt_transform, double radius,
                                                                 int tiles_per_pair, FinePartial* __restrict__ partials) {
  __shared__ float4 tile[kSrcTile];
  __shared__ double dscratch[kFineThreads / 64];
  __shared__ int iscratch[kFineThreads / 64];
  const int p = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int n = selected_rows(corr_offsets, p, limit);
  if (t * kFineThreads >= n) return;  // (uniform over the workgroup)
  const int64_t begin = corr_offsets[p];
  const float* T = gt_transform + 16ll * p;
  const int i = t * kFineThreads + tid;
  const bool live = i < n;
  float rx = 0.f, ry = 0.f, rz = 0.f, residual = 0.f;
  if (live) {
    rx = ref[3 * (begin + i)]; ry = ref[3 * (begin + i) + 1]; rz = ref[3 * (begin + i) + 2];
    const float3 m = move_point(T, src[3 * (begin + i)], src[3 * (begin + i) + 1], src[3 * (begin + i) + 2]);
    const float dx = rx - m.x, dy = ry - m.y, dz = rz - m.z;
    residual = sqrtf((dx * dx + dy * dy) + dz * dz);
  }
  float best = __builtin_inff();
  for (int j0 = 0; j0 < n; j0 += kSrcTile) {
    const int m = n - j0 < kSrcTile ? n - j0 : kSrcTile;
    __syncthreads();
    for (int j = tid; j < m; j += kFineThreads) {
      const float* s = src + 3 * (begin + j0 + j);
      const float3 q = move_point(T, s[0], s[1], s[2]);
      tile[j] = make_float4(q.x, q.y, q.z, 0.f);
    }
    __syncthreads();
    if (live) {
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const float4 q = tile[j];  // same address in every lane: one broadcast read
        const float dx = rx - q.x, dy = ry - q.y, dz = rz - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        best = d2 < best ? d2 : best;
      }
    }
  }
  const float r32 = static_cast<float>(radius);
  const int c0 = block_sum_i<kFineThreads>(live && residual < r32 ? 1 : 0, iscratch);
  const int c1 = block_sum_i<kFineThreads>(live && residual < 0.3f ? 1 : 0, iscratch);
  const int c2 = block_sum_i<kFineThreads>(live && residual < 0.1f ? 1 : 0, iscratch);
  const int ov = block_sum_i<kFineThreads>(live && sqrt(static_cast<double>(best)) < radius ? 1 : 0, iscratch);
  const double rs = block_sum<kFineThreads>(live ? static_cast<double>(residual) : 0.0, dscratch);
  if (tid == 0) {
    FinePartial& o = partials[static_cast<int64_t>(p) * tiles_per_pair + t];
    o.residual_sum = rs;
    o.inliers[0] = c0; o.inliers[1] = c1; o.inliers[2] = c2;
    o.overlap = ov;
  }
}

// ----------------------------------------------------------------------------------------------------------- finish
// registration.py:36-53: degrees with the reference's literal pi
__device__ inline void euler_degrees(const double R[9], double e[3]) {
  const double sy = sqrt(R[0] * R[0] + R[3] * R[3]);
  if (sy >= 1e-6) {
    e[0] = atan2(R[7], R[8]); e[1] = atan2(-R[6], sy); e[2] = atan2(R[3], R[0]);
  } else {
    e[0] = atan2(-R[5], R[4]); e[1] = atan2(-R[6], sy); e[2] = 0.0;
  }
  for (int k = 0; k < 3; ++k) e[k] = e[k] * 180.0 / 3.141592653589793;
}

// One workgroup per pair.  Coarse precision (registration.py:378-402): the M x N cells in rounds of kCellChunk; per round
// two byte maps in LDS, ground truth and predicted, filled with plain stores of 1 (a cell named twice is stored twice, the
// same value), then counted four cells per word.  Then thread 0: the tiles' partials in tile order, the registration
// error in float64, the record.
__global__ __launch_bounds__(kFinishThreads) void eval_finish_kernel(
    const int64_t* __restrict__ corr_offsets, int limit, const float* __restrict__ gt_transform, const float* __restrict__ est,
    const int64_t* __restrict__ node_offsets, const int64_t* __restrict__ ref_node, const int64_t* __restrict__ src_node,
    const int64_t* __restrict__ gt_offsets, const int64_t* __restrict__ gt_node, const int64_t* __restrict__ node_dims,
    int tiles_per_pair, const FinePartial* __restrict__ partials, double* __restrict__ records) {
  __shared__ uint32_t gt_map[kCellChunk / 4], pred_map[kCellChunk / 4];
  __shared__ int iscratch[kFinishThreads / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t M = node_dims[2 * p], N = node_dims[2 * p + 1], cells = M * N;
  const int64_t pb = node_offsets[p], pe = node_offsets[p + 1], gb = gt_offsets[p], ge = gt_offsets[p + 1];
  unsigned char* gt_bytes = reinterpret_cast<unsigned char*>(gt_map);
  unsigned char* pred_bytes = reinterpret_cast<unsigned char*>(pred_map);
  int hit = 0, pred = 0, gt = 0, bad = 0;
  for (int64_t c0 = 0; c0 < cells; c0 += kCellChunk) {
    __syncthreads();
    for (int w = tid; w < kCellChunk / 4; w += kFinishThreads) {
      gt_map[w] = 0u;
      pred_map[w] = 0u;
    }
    __syncthreads();
    for (int64_t k = gb + tid; k < ge; k += kFinishThreads) {
      const int64_t r = gt_node[2 * k], s = gt_node[2 * k + 1];
      const bool ok = r >= 0 && r < M && s >= 0 && s < N;
      const int64_t cell = r * N + s - c0;
      if (ok && cell >= 0 && cell < kCellChunk) gt_bytes[cell] = 1;
      if (!ok && c0 == 0) ++bad;
    }
    for (int64_t k = pb + tid; k < pe; k += kFinishThreads) {
      const int64_t r = ref_node[k], s = src_node[k];
      const bool ok = r >= 0 && r < M && s >= 0 && s < N;
      const int64_t cell = r * N + s - c0;
      if (ok && cell >= 0 && cell < kCellChunk) pred_bytes[cell] = 1;
      if (!ok && c0 == 0) ++bad;
    }
    __syncthreads();
    for (int w = tid; w < kCellChunk / 4; w += kFinishThreads) {
      const uint32_t g = gt_map[w], q = pred_map[w];
      gt += __popc(g);
      pred += __popc(q);
      hit += __popc(g & q);
    }
  }
  hit = block_sum_i<kFinishThreads>(hit, iscratch);
  pred = block_sum_i<kFinishThreads>(pred, iscratch);
  gt = block_sum_i<kFinishThreads>(gt, iscratch);
  bad = block_sum_i<kFinishThreads>(bad, iscratch);
  if (tid != 0) return;

  const int n = selected_rows(corr_offsets, p, limit);
  double rs = 0.0;
  long long cnt[4] = {0, 0, 0, 0};
  const int tiles = (n + kFineThreads - 1) / kFineThreads;
  for (int t = 0; t < tiles; ++t) {
    const FinePartial& q = partials[static_cast<int64_t>(p) * tiles_per_pair + t];
    rs += q.residual_sum;
    cnt[0] += q.inliers[0]; cnt[1] += q.inliers[1]; cnt[2] += q.inliers[2]; cnt[3] += q.overlap;
  }
  double* rec = records + static_cast<int64_t>(p) * RDM_EVAL_RECORD_WIDTH;
  const double nan = __builtin_nan("");
  rec[0] = n;
  rec[1] = n > 0 ? rs / n : nan;
  rec[2] = n > 0 ? static_cast<double>(cnt[0]) / n : nan;
  rec[3] = n > 0 ? static_cast<double>(cnt[1]) / n : nan;
  rec[4] = n > 0 ? static_cast<double>(cnt[2]) / n : nan;
  rec[5] = n > 0 ? static_cast<double>(cnt[3]) / n : nan;
  rec[6] = static_cast<double>(hit) / (static_cast<double>(pred) + 1e-12);

  // registration.py:17-108.  The entries are fp32 values, so every product below is exact in float64.
  double G[9], E[9], gtr[3], etr[3];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      G[3 * a + b] = gt_transform[16ll * p + 4 * a + b];
      E[3 * a + b] = est[16ll * p + 4 * a + b];
    }
    gtr[a] = gt_transform[16ll * p + 4 * a + 3];
    etr[a] = est[16ll * p + 4 * a + 3];
  }
  double trace = 0.0;
  for (int b = 0; b < 3; ++b) trace += (E[b] * G[b] + E[3 + b] * G[3 + b]) + E[6 + b] * G[6 + b];  // diag(E^T G)
  double x = 0.5 * (trace - 1.0);
  x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
  rec[7] = 180.0 * acos(x) / 3.14159265358979323846;
  const double dx = gtr[0] - etr[0], dy = gtr[1] - etr[1], dz = gtr[2] - etr[2];
  rec[8] = sqrt((dx * dx + dy * dy) + dz * dz);
  double ge3[3], ee3[3];
  euler_degrees(G, ge3);
  euler_degrees(E, ee3);
  for (int k = 0; k < 3; ++k) rec[9 + k] = fabs(ge3[k] - ee3[k]);
  for (int k = 0; k < 4; ++k) rec[12 + k] = static_cast<double>(cnt[k]);
  rec[16] = hit;
  rec[17] = pred;
  rec[18] = gt;
  rec[19] = bad;
}

struct Plan {
  bool select;
  int tiles;
  size_t ransac_bytes;
};

Plan make_plan(int64_t max_corr, const rdm_eval_options* o) {
  Plan pl;
  pl.select = o->num_corr > 0 && max_corr > o->num_corr;
  const int64_t rows = pl.select ? o->num_corr : max_corr;
  pl.tiles = static_cast<int>(rows > 0 ? (rows + kFineThreads - 1) / kFineThreads : 1);
  pl.ransac_bytes = o->method == RDM_EVAL_RANSAC ? rdm_ransac_workspace_bytes(o->ransac_iterations) : 0;
  return pl;
}

}  // namespace

extern "C" size_t rdm_eval_pairs_workspace_bytes(int64_t num_pairs, int64_t total_corr, int64_t max_corr,
                                                 const rdm_eval_options* options) {
  using namespace rdm;
  if (!options || num_pairs < 0 || total_corr < 0 || max_corr < 0) return 0;
  const Plan pl = make_plan(max_corr, options);
  const size_t P = static_cast<size_t>(num_pairs > 0 ? num_pairs : 1), rows = static_cast<size_t>(total_corr > 0 ? total_corr : 1);
  size_t b = align_up(P * pl.tiles * sizeof(FinePartial));
  if (pl.select) b += 2 * align_up(rows * 3 * sizeof(float)) + align_up(rows * sizeof(float));
  if (options->method == RDM_EVAL_RANSAC)
    b += align_up(pl.ransac_bytes) + align_up(P * 2 * sizeof(int32_t)) + align_up(P * sizeof(float));
  return b;
}

extern "C" int rdm_eval_pairs(int64_t num_pairs, const int64_t* corr_offsets, const int64_t* corr_offsets_host,
                              const float* ref_corr, const float* src_corr, const float* corr_scores, const float* gt_transform,
                              float* est_transform, const int64_t* node_offsets, const int64_t* ref_node_corr,
                              const int64_t* src_node_corr, const int64_t* gt_offsets, const int64_t* gt_node_corr,
                              const int64_t* node_dims, const rdm_eval_options* options, double* records, void* ws,
                              size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(options && corr_offsets && corr_offsets_host && gt_transform && est_transform && node_offsets && gt_offsets &&
                  node_dims && records,
              "rdm_eval_pairs: null argument");
  RDM_REQUIRE(num_pairs >= 0 && num_pairs <= 65535, "rdm_eval_pairs: 0 <= num_pairs <= 65535 (got %lld)",
              static_cast<long long>(num_pairs));
  RDM_REQUIRE(options->method >= RDM_EVAL_LGR && options->method <= RDM_EVAL_RANSAC && options->num_corr >= 0 &&
                  options->acceptance_radius > 0.0,
              "rdm_eval_pairs: bad options");
  if (num_pairs == 0) return RDM_OK;
  const int P = static_cast<int>(num_pairs);
  int64_t max_corr = 0;
  RDM_REQUIRE(corr_offsets_host[0] == 0, "rdm_eval_pairs: corr_offsets must start at 0");
  for (int p = 0; p < P; ++p) {
    const int64_t c = corr_offsets_host[p + 1] - corr_offsets_host[p];
    RDM_REQUIRE(c >= 0 && c < (1ll << 30), "rdm_eval_pairs: pair %d has %lld correspondences", p, static_cast<long long>(c));
    max_corr = c > max_corr ? c : max_corr;
  }
  const int64_t total = corr_offsets_host[P];
  RDM_REQUIRE(total == 0 || (ref_corr && src_corr && corr_scores), "rdm_eval_pairs: null correspondences");
  const Plan pl = make_plan(max_corr, options);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  FinePartial* partials = ar.take<FinePartial>(static_cast<size_t>(P) * pl.tiles);
  const float *ref = ref_corr, *src = src_corr, *scores = corr_scores;
  float *sel_ref = nullptr, *sel_src = nullptr, *sel_scores = nullptr;
  if (pl.select) {
    const size_t rows = static_cast<size_t>(total);
    sel_ref = ar.take<float>(rows * 3);
    sel_src = ar.take<float>(rows * 3);
    sel_scores = ar.take<float>(rows);
  }
  void* ransac_ws = nullptr;
  int32_t* ransac_stats = nullptr;
  float* ransac_rmse = nullptr;
  if (options->method == RDM_EVAL_RANSAC) {
    ransac_ws = ar.take<char>(pl.ransac_bytes);
    ransac_stats = ar.take<int32_t>(static_cast<size_t>(P) * 2);
    ransac_rmse = ar.take<float>(P);
  }
  if (!ar.ok) {
    set_error("rdm_eval_pairs: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  const int limit = options->num_corr;
  if (pl.select) {
    hipLaunchKernelGGL(eval_select_kernel, dim3(P), dim3(kSelectThreads), 0, st, corr_offsets, ref_corr, src_corr, corr_scores,
                       limit, sel_ref, sel_src, sel_scores);
    ref = sel_ref; src = sel_src; scores = sel_scores;
  }
  if (options->method == RDM_EVAL_SVD) {
    hipLaunchKernelGGL(eval_procrustes_kernel, dim3(P), dim3(256), 0, st, corr_offsets, limit, ref, src, scores, est_transform);
  } else if (options->method == RDM_EVAL_RANSAC) {
    for (int p = 0; p < P; ++p) {
      const int64_t begin = corr_offsets_host[p], c = corr_offsets_host[p + 1] - begin;
      const int64_t n = (limit > 0 && c > limit) ? limit : c;
      const int rc = rdm_ransac_correspondences(src ? src + 3 * begin : nullptr, ref ? ref + 3 * begin : nullptr, n,
                                                options->ransac_distance_threshold, options->ransac_n,
                                                options->ransac_iterations, options->ransac_seed, est_transform + 16ll * p,
                                                ransac_stats + 2 * p, ransac_rmse + p, nullptr, ransac_ws, pl.ransac_bytes, st);
      if (rc != RDM_OK) return rc;
    }
  }
  if (max_corr > 0)
    hipLaunchKernelGGL(eval_fine_kernel, dim3(pl.tiles, P), dim3(kFineThreads), 0, st, corr_offsets, limit, ref, src,
                       gt_transform, options->acceptance_radius, pl.tiles, partials);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(P), dim3(kFinishThreads), 0, st, corr_offsets, limit, gt_transform,
                     static_cast<const float*>(est_transform), node_offsets, ref_node_corr, src_node_corr, gt_offsets,
                     gt_node_corr, node_dims, pl.tiles, partials, records);
  return launch_status("rdm_eval_pairs");
}
