// Descriptor matching: for every row of a [N, C] its nearest row of b [M, C] under the L2 distance (and the mirror image with
// both_sides), the answer being the float64 brute-force one -- argmin_j sum_c (a_ic - b_jc)^2 evaluated in double on the fp32
// inputs, lowest index among exactly equal distances.  Replaces get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22,
// a cKDTree in C dimensions) as extract_corr_indices_from_feats uses it (geotransformer/utils/registration.py:222-255).
//
// Phase 1 (fm_tile_kernel) forms e_ij = fl(fl(na_i + nb_j) - 2 dot_ij) per 128 x 128 tile on v_mfma_f32_32x32x2_f32, operands
// staged through LDS, and keeps per line (row, and column with both_sides) of the tile the best candidate (e1, j1) and the second
// smallest value e2; the N x M values never leave the registers.  The per-tile triples are ordered partials: fm_reduce_kernel
// merges them per line in ascending tile order, so nothing depends on scheduling and there are no float atomics.
//
// The bound.  With u = 2^-24, A = |a_i|^2, B = |b_j|^2 (exact), na / nb their fp32 roundings (summed in double, so one rounding:
// |na - A| <= u A), dot an fp32 fma chain over C products (|dot - a.b| <= g sum|a_c b_c| <= g (A + B) / 2, g = C u / (1 - C u)),
// s = fl(na + nb) and e = fl(s - 2 dot) (2 dot is exact, fmaf rounds once):
//   e - d = (na - A) + (nb - B) + d2 (na + nb) - 2 (dot - a.b) + d3 (s - 2 dot),  |d2|, |d3| <= u,
//   |e - d| <= u A + u B + u (1 + u)(A + B) + g (A + B) + u (2 + 3 u + g)(A + B)  <  (C + 5)(1 + 2^-10) u (A + B)   for C <= 1024.
// E_i = (C + 8) u (na_i + max_j nb_j) + 2^-100 covers it for every j of line i (the 3 u of slack absorb na, nb standing in for A, B
// and the second-order terms; 2^-100 the absolute error of products that underflow, at most C 2^-150).  If e2 - e1 > 2 E_i then for
// every j != j1: d_j >= e_j - E >= e2 - E > e1 + E >= d_j1, so j1 is the unique float64 argmin.  Otherwise the line goes to
// phase 2 (fm_exact_kernel), which evaluates the direct difference form in float64 -- one fma chain over ascending c -- for EVERY j
// of that line (the widest candidate set: nothing has to be certified about the fp32 values of the others) and keeps the smallest
// (distance, index).  An e that overflowed or is NaN fails the test above and takes phase 2 as well.
// fm_finish_kernel writes the index and sqrt(float64 sum) rounded to fp32 for every line.
#include "common.h"
#include "../../include/rdmnet_hip.h"

#include <algorithm>
#include <climits>

namespace rdm {
namespace {

constexpr int kTile = 128;     // rows and columns of a phase-1 tile (4 wavefronts, 64 x 64 each)
constexpr int kKT = 16;        // k-tile depth
constexpr int kLd = kKT + 1;   // LDS row stride (floats)
constexpr int kLines = 8;      // phase 2: lines per workgroup
constexpr int kChunk = 256;    // phase 2: candidates per pass (one per thread)
constexpr int kMaxSplits = 64; // phase 2: candidate ranges per line

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Top2 {  // best candidate and the second smallest value of a set
  float e1;
  int j1;
  float e2;
};
__device__ __forceinline__ Top2 top2_empty() { return Top2{INFINITY, INT_MAX, INFINITY}; }
__device__ __forceinline__ void top2_add(Top2& x, float e, int j) {
  if (e < x.e1 || (e == x.e1 && j < x.j1)) {
    x.e2 = x.e1; x.e1 = e; x.j1 = j;
  } else if (e < x.e2) {
    x.e2 = e;
  }
}
__device__ __forceinline__ void top2_merge(Top2& x, const Top2& y) {
  if (y.e1 < x.e1 || (y.e1 == x.e1 && y.j1 < x.j1)) {
    const float o = x.e1;
    x.e1 = y.e1; x.j1 = y.j1;
    x.e2 = o < y.e2 ? o : y.e2;
  } else if (y.e1 < x.e2) {
    x.e2 = y.e1;
  }
}
__device__ __forceinline__ Top2 top2_shfl_xor(const Top2& x, int mask) {
  Top2 y;
  y.e1 = __shfl_xor(x.e1, mask, 64);
  y.j1 = __shfl_xor(x.j1, mask, 64);
  y.e2 = __shfl_xor(x.e2, mask, 64);
  return y;
}

// 8 consecutive floats of row `row` from column k (zeros outside the matrix)
template <bool VEC>
__device__ __forceinline__ void load8(const float* __restrict__ p, int64_t ld, int64_t row, int64_t nrows, int k, int C, float (&v)[8]) {
  if (VEC) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (row < nrows) {
      const float* q = p + row * ld + k;
      if (k < C) x = *reinterpret_cast<const float4*>(q);
      if (k + 4 < C) y = *reinterpret_cast<const float4*>(q + 4);
    }
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = (row < nrows && k + t < C) ? p[row * ld + k + t] : 0.f;
  }
}

// |x_r|^2 summed in double, rounded once, for the rows of a then b; the largest of each side as the bits of a non-negative float
__global__ __launch_bounds__(256) void fm_norm_kernel(const float* __restrict__ a, int64_t lda, int64_t n, const float* __restrict__ b,
                                                      int64_t ldb, int64_t m, int C, float* __restrict__ na, float* __restrict__ nb,
                                                      unsigned* __restrict__ maxbits) {
  const int64_t w = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (w >= n + m) return;
  const bool is_b = w >= n;
  const float* row = is_b ? b + (w - n) * ldb : a + w * lda;
  double s = 0.0;
  for (int c = lane_id(); c < C; c += 64) {
    const double v = row[c];
    s = fma(v, v, s);
  }
  s = wave_sum(s);
  if (lane_id() == 0) {
    const float f = static_cast<float>(s);
    (is_b ? nb[w - n] : na[w]) = f;
    if (f == f) atomicMax(maxbits + (is_b ? 1 : 0), __float_as_uint(f));  // (integer atomic on the bits of a float >= 0)
  }
}

struct TileArgs {
  const float *a, *b, *na, *nb;
  int64_t lda, ldb;
  int n, m, C;
  int row_parts, col_parts;  // tiles per row (= column blocks) and per column (= row blocks)
  float *row_e1, *row_e2, *col_e1, *col_e2;
  int *row_j1, *col_j1;      // col_*: null without both_sides
};

template <bool VEC>
__global__ __launch_bounds__(256) void fm_tile_kernel(TileArgs g) {
  __shared__ float As[kTile * kLd], Bs[kTile * kLd];
  __shared__ Top2 s_row[2][kTile], s_col[2][kTile];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bm = blockIdx.y * kTile, bn = blockIdx.x * kTile;
  const int lr = t >> 1, lk = (t & 1) * 8;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float ra[8], rb[8];
  load8<VEC>(g.a, g.lda, bm + lr, g.n, lk, g.C, ra);
  load8<VEC>(g.b, g.ldb, bn + lr, g.m, lk, g.C, rb);
  const int a_off = (wr * 64 + (lane & 31)) * kLd + (lane >> 5);
  const int b_off = (wc * 64 + (lane & 31)) * kLd + (lane >> 5);
  for (int k0 = 0; k0 < g.C; k0 += kKT) {
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      As[lr * kLd + lk + x] = ra[x];
      Bs[lr * kLd + lk + x] = rb[x];
    }
    __syncthreads();
    if (k0 + kKT < g.C) {  // the next k-tile's rows travel while this one is multiplied
      load8<VEC>(g.a, g.lda, bm + lr, g.n, k0 + kKT + lk, g.C, ra);
      load8<VEC>(g.b, g.ldb, bn + lr, g.m, k0 + kKT + lk, g.C, rb);
    }
#pragma unroll
    for (int s = 0; s < kKT / 2; ++s) {
      // lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31] of the 32 x 32 x 2 product
      const float a0 = As[a_off + 2 * s], a1 = As[a_off + 32 * kLd + 2 * s];
      const float b0 = Bs[b_off + 2 * s], b1 = Bs[b_off + 32 * kLd + 2 * s];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // e = fl(fl(na + nb) - 2 dot); element (reg, lane) of a 32 x 32 result: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int half = lane >> 5;
  int col[2];
  float nbv[2];
  bool col_ok[2];
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    col[tj] = bn + wc * 64 + tj * 32 + (lane & 31);
    col_ok[tj] = col[tj] < g.m;
    nbv[tj] = col_ok[tj] ? g.nb[col[tj]] : 0.f;
  }
  Top2 cbest[2] = {top2_empty(), top2_empty()};
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lrow = wr * 64 + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      const int row = bm + lrow;
      const bool row_ok = row < g.n;
      const float nav = row_ok ? g.na[row] : 0.f;
      Top2 x = top2_empty();
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const float e = fmaf(-2.f, acc[ti][tj][r], nav + nbv[tj]);
        if (row_ok && col_ok[tj]) {
          top2_add(x, e, col[tj]);
          top2_add(cbest[tj], e, row);
        }
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) top2_merge(x, top2_shfl_xor(x, o));  // over the 32 columns held by this half's lanes
      if ((lane & 31) == 0) s_row[wc][lrow] = x;
    }
  }
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    top2_merge(cbest[tj], top2_shfl_xor(cbest[tj], 32));  // the other half's rows
    if (half == 0) s_col[wr][wc * 64 + tj * 32 + lane] = cbest[tj];
  }
  __syncthreads();
  if (t < kTile) {
    Top2 x = s_row[0][t];
    top2_merge(x, s_row[1][t]);
    if (bm + t < g.n) {
      const int64_t o = static_cast<int64_t>(bm + t) * g.row_parts + blockIdx.x;
      g.row_e1[o] = x.e1; g.row_j1[o] = x.j1; g.row_e2[o] = x.e2;
    }
  } else if (g.col_e1 != nullptr) {
    const int c = t - kTile;
    Top2 x = s_col[0][c];
    top2_merge(x, s_col[1][c]);
    if (bn + c < g.m) {
      const int64_t o = static_cast<int64_t>(bn + c) * g.col_parts + blockIdx.y;
      g.col_e1[o] = x.e1; g.col_j1[o] = x.j1; g.col_e2[o] = x.e2;
    }
  }
}

// One thread per line: the tile partials in ascending tile order, then the certificate (header comment).
__global__ __launch_bounds__(256) void fm_reduce_kernel(const float* __restrict__ pe1, const int* __restrict__ pj1,
                                                        const float* __restrict__ pe2, int parts, int lines,
                                                        const float* __restrict__ norm_self, const unsigned* __restrict__ max_other,
                                                        int C, int64_t* __restrict__ idx, int* __restrict__ slot, int* __restrict__ list,
                                                        int* __restrict__ counter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lines) return;
  Top2 x = top2_empty();
  for (int p = 0; p < parts; ++p) {
    const int64_t o = static_cast<int64_t>(i) * parts + p;
    top2_merge(x, Top2{pe1[o], pj1[o], pe2[o]});
  }
  const double bound = (C + 8) * 0x1p-24 * (static_cast<double>(norm_self[i]) + static_cast<double>(__uint_as_float(*max_other))) + 0x1p-100;
  const bool certain = x.j1 != INT_MAX && static_cast<double>(x.e2) - static_cast<double>(x.e1) > 2.0 * bound;
  if (certain) {
    idx[i] = x.j1;
    slot[i] = -1;
  } else {
    const int s = atomicAdd(counter, 1);  // (the order of the list is arbitrary; every line's result lands in its own place)
    list[s] = i;
    slot[i] = s;
  }
}

// Phase 2: workgroup (g, split) evaluates sum_c (x_c - y_c)^2 in float64 -- one fma chain over ascending c -- between kLines listed
// lines of `self` and every row of `other` in its candidate range, and writes the smallest (distance, index) per line.
template <bool VEC>
__global__ __launch_bounds__(kChunk) void fm_exact_kernel(const float* __restrict__ self, int64_t ld_self, const float* __restrict__ other,
                                                          int64_t ld_other, int n_other, int C, int Cpad, const int* __restrict__ list,
                                                          const int* __restrict__ counter, int splits, int range,
                                                          double* __restrict__ part_d, int* __restrict__ part_j) {
  extern __shared__ __align__(16) float s_self[];  // [kLines][Cpad], zero padded
  __shared__ float Bs[kChunk * kLd];
  __shared__ double s_d[kChunk / 64][kLines];
  __shared__ int s_j[kChunk / 64][kLines];
  const int count = *counter;
  const int slot0 = blockIdx.x * kLines;
  if (slot0 >= count) return;
  const int t = threadIdx.x;
  for (int l = 0; l < kLines; ++l) {
    const int line = list[min(slot0 + l, count - 1)];
    for (int c = t; c < Cpad; c += kChunk) s_self[l * Cpad + c] = c < C ? self[static_cast<int64_t>(line) * ld_self + c] : 0.f;
  }
  double best[kLines];
  int best_j[kLines];
#pragma unroll
  for (int l = 0; l < kLines; ++l) { best[l] = INFINITY; best_j[l] = 0; }
  const int j_begin = blockIdx.y * range, j_end = min(n_other, j_begin + range);
  const int lr = t >> 1, lk = (t & 1) * 8;
  for (int j0 = j_begin; j0 < j_end; j0 += kChunk) {
    double acc[kLines];
#pragma unroll
    for (int l = 0; l < kLines; ++l) acc[l] = 0.0;
    for (int k0 = 0; k0 < C; k0 += kKT) {
      float r0[8], r1[8];
      load8<VEC>(other, ld_other, j0 + lr, j_end, k0 + lk, C, r0);
      load8<VEC>(other, ld_other, j0 + 128 + lr, j_end, k0 + lk, C, r1);
      __syncthreads();
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        Bs[lr * kLd + lk + x] = r0[x];
        Bs[(128 + lr) * kLd + lk + x] = r1[x];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kKT / 4; ++q) {
        double y[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) y[x] = Bs[t * kLd + 4 * q + x];
#pragma unroll
        for (int l = 0; l < kLines; ++l) {
          const float4 xv = *reinterpret_cast<const float4*>(&s_self[l * Cpad + k0 + 4 * q]);
          double d = static_cast<double>(xv.x) - y[0];
          acc[l] = fma(d, d, acc[l]);
          d = static_cast<double>(xv.y) - y[1];
          acc[l] = fma(d, d, acc[l]);
          d = static_cast<double>(xv.z) - y[2];
          acc[l] = fma(d, d, acc[l]);
          d = static_cast<double>(xv.w) - y[3];
          acc[l] = fma(d, d, acc[l]);
        }
      }
    }
    const int j = j0 + t;
    if (j < j_end) {
#pragma unroll
      for (int l = 0; l < kLines; ++l)
        if (acc[l] < best[l]) { best[l] = acc[l]; best_j[l] = j; }  // (a thread's j ascend: the lowest index of equals stays)
    }
  }
#pragma unroll
  for (int l = 0; l < kLines; ++l) {
    double d = best[l];
    int j = best_j[l];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double d2 = __shfl_xor(d, o, 64);
      const int j2 = __shfl_xor(j, o, 64);
      if (d2 < d || (d2 == d && j2 < j)) { d = d2; j = j2; }
    }
    if ((t & 63) == 0) { s_d[t >> 6][l] = d; s_j[t >> 6][l] = j; }
  }
  __syncthreads();
  if (t < kLines && slot0 + t < count) {
    double d = s_d[0][t];
    int j = s_j[0][t];
    for (int w = 1; w < kChunk / 64; ++w)
      if (s_d[w][t] < d || (s_d[w][t] == d && s_j[w][t] < j)) { d = s_d[w][t]; j = s_j[w][t]; }
    const int64_t o = static_cast<int64_t>(slot0 + t) * splits + blockIdx.y;
    part_d[o] = d;
    part_j[o] = j;
  }
}

// One wavefront per line: the index (phase 2's where the line took it) and the distance sqrt(float64 sum) rounded to fp32.
__global__ __launch_bounds__(256) void fm_finish_kernel(const float* __restrict__ self, int64_t ld_self, const float* __restrict__ other,
                                                        int64_t ld_other, int lines, int C, const int* __restrict__ slot, int splits,
                                                        const double* __restrict__ part_d, const int* __restrict__ part_j,
                                                        int64_t* __restrict__ idx, float* __restrict__ dist) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= lines) return;
  const int s = slot[i];
  double d;
  if (s >= 0) {
    d = INFINITY;
    int j = 0;
    for (int p = 0; p < splits; ++p) {  // (ascending ranges: strict < keeps the lowest index)
      const double dp = part_d[static_cast<int64_t>(s) * splits + p];
      if (dp < d) { d = dp; j = part_j[static_cast<int64_t>(s) * splits + p]; }
    }
    if (lane_id() == 0) idx[i] = j;
  } else {
    const float* x = self + static_cast<int64_t>(i) * ld_self;
    const float* y = other + idx[i] * ld_other;
    d = 0.0;
    for (int c = lane_id(); c < C; c += 64) {
      const double v = static_cast<double>(x[c]) - static_cast<double>(y[c]);
      d = fma(v, v, d);
    }
    d = wave_sum(d);
  }
  if (lane_id() == 0 && dist != nullptr) dist[i] = static_cast<float>(sqrt(d));
}

// mode 0: (arange(N), nn_ab); 2: ([arange(N), nn_ba], [nn_ab, arange(M)]); the distances alongside
__global__ __launch_bounds__(256) void fm_select_plain_kernel(int mode, const int64_t* __restrict__ nn_ab, const float* __restrict__ d_ab,
                                                              const int64_t* __restrict__ nn_ba, const float* __restrict__ d_ba, int64_t n,
                                                              int64_t m, int64_t* __restrict__ ref_idx, int64_t* __restrict__ src_idx,
                                                              float* __restrict__ dist, int32_t* __restrict__ count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = mode == 2 ? n + m : n;
  if (i == 0) *count = static_cast<int32_t>(total);
  if (i >= total) return;
  if (i < n) {
    ref_idx[i] = i; src_idx[i] = nn_ab[i];
    if (dist) dist[i] = d_ab[i];
  } else {
    ref_idx[i] = nn_ba[i - n]; src_idx[i] = i - n;
    if (dist) dist[i] = d_ba[i - n];
  }
}

// mode 1: the rows i with nn_ba[nn_ab[i]] == i in ascending i, by one workgroup (an ordered compaction)
__global__ __launch_bounds__(1024) void fm_select_mutual_kernel(const int64_t* __restrict__ nn_ab, const float* __restrict__ d_ab,
                                                                const int64_t* __restrict__ nn_ba, int64_t n, int64_t* __restrict__ ref_idx,
                                                                int64_t* __restrict__ src_idx, float* __restrict__ dist,
                                                                int32_t* __restrict__ count) {
  __shared__ int s_wave[16];
  __shared__ int s_total;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) s_total = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + t;
    const bool keep = i < n && nn_ba[nn_ab[i]] == i;
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(bal);
    __syncthreads();
    int off = s_total;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (keep) {
      ref_idx[off + before] = i; src_idx[off + before] = nn_ab[i];
      if (dist) dist[off + before] = d_ab[i];
    }
    __syncthreads();
    if (t == 0) {
      int s = s_total;
      for (int w = 0; w < 16; ++w) s += s_wave[w];
      s_total = s;
    }
    __syncthreads();
  }
  if (t == 0) *count = s_total;
}

__global__ __launch_bounds__(256) void fm_gather_points_kernel(const float* __restrict__ ref_points, const float* __restrict__ src_points,
                                                               const int64_t* __restrict__ ref_idx, const int64_t* __restrict__ src_idx,
                                                               const int32_t* __restrict__ count, float* __restrict__ ref_out,
                                                               float* __restrict__ src_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= *count) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ref_out[3 * i + c] = ref_points[3 * ref_idx[i] + c];
    src_out[3 * i + c] = src_points[3 * src_idx[i] + c];
  }
}

int splits_of(int64_t n_other) { return static_cast<int>(std::min<int64_t>(kMaxSplits, std::max<int64_t>(1, ceil_div<int64_t>(n_other, 1024)))); }

struct Side {  // the buffers of one direction (lines of `self` against the rows of `other`)
  float *e1, *e2;
  int *j1, *slot, *list, *part_j;
  double* part_d;
};
void take_side(Arena& ar, int64_t lines, int64_t parts, int splits, Side& s) {
  const size_t np = static_cast<size_t>(std::max<int64_t>(lines, 1)) * parts;
  s.e1 = ar.take<float>(np);
  s.e2 = ar.take<float>(np);
  s.j1 = ar.take<int>(np);
  s.slot = ar.take<int>(lines);
  s.list = ar.take<int>(lines);
  s.part_d = ar.take<double>(static_cast<size_t>(lines) * splits);
  s.part_j = ar.take<int>(static_cast<size_t>(lines) * splits);
}

struct Layout {
  float *na, *nb;
  unsigned* words;  // {max |a|^2 bits, max |b|^2 bits, phase-2 lines of a, phase-2 lines of b}
  Side row, col;
};
size_t layout(void* ws, size_t ws_bytes, int64_t n, int64_t m, int both, Layout& L, bool* ok) {
  Arena ar(ws, ws_bytes);
  L.words = ar.take<unsigned>(4);
  L.na = ar.take<float>(n);
  L.nb = ar.take<float>(m);
  take_side(ar, n, ceil_div<int64_t>(m, kTile), splits_of(m), L.row);
  if (both) take_side(ar, m, ceil_div<int64_t>(n, kTile), splits_of(n), L.col);
  if (ok) *ok = ar.ok;
  return ar.off;
}

bool vec_ok(const float* p, int64_t ld, int64_t c) { return c % 4 == 0 && ld % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// reduce, phase 2 and finish of one direction
int resolve_side(const float* self, int64_t ld_self, int lines, const float* norm_self, const float* other, int64_t ld_other, int n_other,
                 const unsigned* max_other, int* counter, int C, bool vec, const Side& s, int parts, int64_t* idx, float* dist,
                 hipStream_t st) {
  hipLaunchKernelGGL(fm_reduce_kernel, dim3(ceil_div(lines, 256)), dim3(256), 0, st, s.e1, s.j1, s.e2, parts, lines, norm_self, max_other, C,
                     idx, s.slot, s.list, counter);
  if (int rc = launch_status("fm_reduce_kernel")) return rc;
  const int splits = splits_of(n_other);
  const int range = ceil_div(ceil_div(n_other, splits), kChunk) * kChunk;
  const int Cpad = ceil_div(C, kKT) * kKT;
  const dim3 grid(ceil_div(lines, kLines), splits);  // (the number of listed lines stays on the device: groups past it return at once)
  const size_t lds = sizeof(float) * kLines * Cpad;
  if (vec) hipLaunchKernelGGL(fm_exact_kernel<true>, grid, dim3(kChunk), lds, st, self, ld_self, other, ld_other, n_other, C, Cpad, s.list,
                              counter, splits, range, s.part_d, s.part_j);
  else hipLaunchKernelGGL(fm_exact_kernel<false>, grid, dim3(kChunk), lds, st, self, ld_self, other, ld_other, n_other, C, Cpad, s.list,
                          counter, splits, range, s.part_d, s.part_j);
  if (int rc = launch_status("fm_exact_kernel")) return rc;
  hipLaunchKernelGGL(fm_finish_kernel, dim3(ceil_div(lines, 4)), dim3(256), 0, st, self, ld_self, other, ld_other, lines, C, s.slot, splits,
                     s.part_d, s.part_j, idx, dist);
  return launch_status("fm_finish_kernel");
}

}  // namespace
}  // namespace rdm

using namespace rdm;

extern "C" size_t rdm_feature_match_workspace_bytes(int64_t n, int64_t m, int both_sides) {
  if (n < 0 || m < 0) return 0;
  Layout L;
  return layout(nullptr, 0, n, m, both_sides, L, nullptr) + 256;
}

extern "C" int rdm_feature_match(const float* a, int64_t lda, int64_t n, const float* b, int64_t ldb, int64_t m, int64_t c, int both_sides,
                                 int64_t* nn_ab, float* dist_ab, int64_t* nn_ba, float* dist_ba, int32_t* phase2_lines, void* ws,
                                 size_t ws_bytes, void* stream) {
  RDM_REQUIRE(n >= 0 && m >= 0 && n < INT_MAX - kTile && m < INT_MAX - kTile, "rdm_feature_match: n = %lld, m = %lld out of range",
              (long long)n, (long long)m);
  RDM_REQUIRE(m > 0, "rdm_feature_match: m = 0: there is no row of b to match the %lld rows of a to", (long long)n);
  RDM_REQUIRE(c >= 1 && c <= 1024, "rdm_feature_match: c = %lld, supported 1 .. 1024", (long long)c);
  RDM_REQUIRE(!(both_sides && n == 0), "rdm_feature_match: n = 0 with both_sides: there is no row of a to match the rows of b to");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (phase2_lines) fill_words<int32_t>(phase2_lines, 2, 0, st);
    return launch_status("fill_words");
  }
  RDM_REQUIRE(a && b && nn_ab && lda >= c && ldb >= c, "rdm_feature_match: null pointer or row stride below c");
  RDM_REQUIRE(!both_sides || nn_ba, "rdm_feature_match: both_sides without nn_ba");
  RDM_REQUIRE(ceil_div<int64_t>(n, kTile) <= 65535, "rdm_feature_match: n = %lld exceeds 65535 row tiles", (long long)n);
  Layout L;
  bool ok = false;
  layout(ws, ws_bytes, n, m, both_sides, L, &ok);
  if (!ok) {
    set_error("rdm_feature_match: workspace of %zu B, needs %zu B", ws_bytes, rdm_feature_match_workspace_bytes(n, m, both_sides));
    return RDM_ERR_WORKSPACE;
  }
  const int C = static_cast<int>(c), N = static_cast<int>(n), M = static_cast<int>(m);
  const bool vec = vec_ok(a, lda, c) && vec_ok(b, ldb, c);
  fill_words<unsigned>(L.words, 4, 0u, st);
  hipLaunchKernelGGL(fm_norm_kernel, dim3(static_cast<unsigned>(ceil_div<int64_t>(n + m, 4))), dim3(256), 0, st, a, lda, n, b, ldb, m, C, L.na,
                     L.nb, L.words);
  if (int rc = launch_status("fm_norm_kernel")) return rc;
  TileArgs g;
  g.a = a; g.b = b; g.na = L.na; g.nb = L.nb; g.lda = lda; g.ldb = ldb; g.n = N; g.m = M; g.C = C;
  g.row_parts = ceil_div(M, kTile); g.col_parts = ceil_div(N, kTile);
  g.row_e1 = L.row.e1; g.row_e2 = L.row.e2; g.row_j1 = L.row.j1;
  g.col_e1 = both_sides ? L.col.e1 : nullptr; g.col_e2 = both_sides ? L.col.e2 : nullptr; g.col_j1 = both_sides ? L.col.j1 : nullptr;
  const dim3 grid(g.row_parts, g.col_parts);
  if (vec) hipLaunchKernelGGL(fm_tile_kernel<true>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(fm_tile_kernel<false>, grid, dim3(256), 0, st, g);
  if (int rc = launch_status("fm_tile_kernel")) return rc;
  int* counters = reinterpret_cast<int*>(L.words + 2);
  if (int rc = resolve_side(a, lda, N, L.na, b, ldb, M, L.words + 1, counters, C, vec, L.row, g.row_parts, nn_ab, dist_ab, st)) return rc;
  if (both_sides)
    if (int rc = resolve_side(b, ldb, M, L.nb, a, lda, N, L.words, counters + 1, C, vec, L.col, g.col_parts, nn_ba, dist_ba, st)) return rc;
  if (phase2_lines) copy_words(counters, phase2_lines, 2, st);
  return launch_status("rdm_feature_match");
}

extern "C" int rdm_feature_match_select(int mode, const int64_t* nn_ab, const float* dist_ab, const int64_t* nn_ba, const float* dist_ba,
                                        int64_t n, int64_t m, int64_t* ref_idx, int64_t* src_idx, float* dist, int32_t* count,
                                        void* stream) {
  RDM_REQUIRE(mode >= 0 && mode <= 2, "rdm_feature_match_select: mode %d (0 nearest, 1 mutual, 2 bilateral)", mode);
  RDM_REQUIRE(n >= 0 && m >= 0 && n + m < INT_MAX, "rdm_feature_match_select: n = %lld, m = %lld out of range", (long long)n, (long long)m);
  RDM_REQUIRE(count && (n == 0 || (nn_ab && ref_idx && src_idx)), "rdm_feature_match_select: null pointer");
  RDM_REQUIRE(mode == 0 || n == 0 || nn_ba, "rdm_feature_match_select: mode %d needs nn_ba", mode);
  RDM_REQUIRE(!dist || n == 0 || (dist_ab && (mode != 2 || dist_ba)), "rdm_feature_match_select: dist without the input distances");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == 1) {
    hipLaunchKernelGGL(fm_select_mutual_kernel, dim3(1), dim3(1024), 0, st, nn_ab, dist_ab, nn_ba, n, ref_idx, src_idx, dist, count);
  } else {
    const int64_t total = std::max<int64_t>(mode == 2 ? n + m : n, 1);
    hipLaunchKernelGGL(fm_select_plain_kernel, dim3(static_cast<unsigned>(ceil_div<int64_t>(total, 256))), dim3(256), 0, st, mode, nn_ab,
                       dist_ab, nn_ba, dist_ba, n, m, ref_idx, src_idx, dist, count);
  }
  return launch_status("rdm_feature_match_select");
}

namespace rdm {
// the correspondences' points (count on the device): used by rdm_engine_feature_correspondences
int feature_match_gather_points(const float* ref_points, const float* src_points, const int64_t* ref_idx, const int64_t* src_idx,
                                const int32_t* count, int64_t capacity, float* ref_out, float* src_out, hipStream_t st) {
  if (capacity <= 0) return RDM_OK;
  hipLaunchKernelGGL(fm_gather_points_kernel, dim3(static_cast<unsigned>(ceil_div<int64_t>(capacity, 256))), dim3(256), 0, st, ref_points,
                     src_points, ref_idx, src_idx, count, ref_out, src_out);
  return launch_status("fm_gather_points_kernel");
}
}  // namespace rdm
