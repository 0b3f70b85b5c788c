// Robust pose from correspondences: compatibility graph, core numbers, maximum clique, GNC-TLS rotation and truncated-
// least-squares translation voting -- the estimator experiments/eval.py:198-219 names `teaser`.
//
// The library that file calls is not under the reference tree -> PARITY UNPINNED.  The definition is this project's own,
// after the published algorithm (Yang, Shi, Carlone: TEASER, 2020), stated in include/rdmnet_hip.h and DESIGN.md section 7
// and restated in float64 numpy by tests/robust_restatement.py.
//
// Structure (C rows, W = ceil(C / 64) words per adjacency row):
//   graph      one wavefront per row: lane l tests column 64 w + l, the ballot IS adjacency word w.
//   core       one block peels the graph: level k removes every live vertex of degree <= k until none is left, then k + 1;
//              removed vertices decrement their live neighbours (integer atomics on the degrees; the core numbers do not depend
//              on the order).
//   greedy     one block: repeatedly the candidate of highest core number (lowest row among equals) -> lower bound LB.
//   search     one wavefront per subproblem v (cliques whose lowest row is v) over the rows of core number >= LB - 1: depth first
//              in ascending row order on bitsets, a lane owns words lane, lane + 64, ... of every level, bound |clique| +
//              popcount(candidates); accepts a first clique of size >= LB, then strictly larger ones; counts its nodes against the
//              budget in the loop condition.  A subproblem uses nothing another one finds.  The stacks come out of a fixed pool:
//              the number of search waves is pool / (depth cap = max core + 2 levels), at least one.
//   select     one block: largest size, then lowest v (or the rows of maximum core number / all rows) -> ascending row list.
//   GNC        per iteration: weighted sum of a b^T over the pairs (block slabs) -> one-thread Horn solve -> residual cost and
//              maximum (block slabs) -> one-thread decision.  Weights are not stored: the weight of a pair is a function of its
//              residual under the previous rotation and the previous thresholds, recomputed with the same arithmetic.
//   translate  per axis: values, rank sort of the 2K interval ends, one thread per midpoint (sums over k ascending), argmin.
// Determinism: lanes by butterfly, waves and slabs in index order, no float atomics.
#include "../../include/rdmnet_hip.h"
#include "common.h"
#include "procrustes.h"

#pragma clang fp contract(off)

namespace {
using namespace rdm;

constexpr int kBlock = 256;
constexpr int kOne = 1024;            // threads of the one-block kernels
constexpr int kMaxW = RDM_ROBUST_MAX_CORR / 64;
constexpr int kPairBlocks = 512;      // blocks (slab rows) of the pair kernels
constexpr int kSearchWaves = 1024;    // at most this many search wavefronts
constexpr size_t kPoolBytes = size_t(256) << 20;
constexpr int kChunk = 16;            // GNC iterations between two reads of `done`
constexpr long long kDefaultCliqueNodes = 65536;  // about one second when every subproblem of 5471 rows runs out

using u64 = unsigned long long;

struct RobustState {
  double R[9];     // the latest solved rotation
  double Rw[9];    // the rotation whose residuals define the current weights
  double th1, th2, muw;  // thresholds and mu of the current weights
  double mu, prev_cost;
  int unit_weights;  // 1: every weight is 1
  int K, valid, exhausted, iterations, done;
  int lb, maxcore, edges, n_waves, depth_cap;
};

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// ---- (1) compatibility graph -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void graph_kernel(const float* __restrict__ src, const float* __restrict__ ref, int C, int W,
                                                       double thr, u64* __restrict__ adj, int32_t* __restrict__ degree) {
  const int row = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= C) return;
  const float sf[3] = {src[3 * row], src[3 * row + 1], src[3 * row + 2]}, rf[3] = {ref[3 * row], ref[3 * row + 1], ref[3 * row + 2]};
  const bool fin_i = isfinite(sf[0]) && isfinite(sf[1]) && isfinite(sf[2]) && isfinite(rf[0]) && isfinite(rf[1]) && isfinite(rf[2]);
  int deg = 0;
  for (int w = 0; w < W; ++w) {
    const int j = 64 * w + lane;
    bool ok = false;
    if (j < C && j != row && fin_i) {
      const float sj[3] = {src[3 * j], src[3 * j + 1], src[3 * j + 2]}, rj[3] = {ref[3 * j], ref[3 * j + 1], ref[3 * j + 2]};
      if (isfinite(sj[0]) && isfinite(sj[1]) && isfinite(sj[2]) && isfinite(rj[0]) && isfinite(rj[1]) && isfinite(rj[2])) {
        const double ax = static_cast<double>(sj[0]) - sf[0], ay = static_cast<double>(sj[1]) - sf[1],
                     az = static_cast<double>(sj[2]) - sf[2];
        const double bx = static_cast<double>(rj[0]) - rf[0], by = static_cast<double>(rj[1]) - rf[1],
                     bz = static_cast<double>(rj[2]) - rf[2];
        const double ds = sqrt(((ax * ax) + (ay * ay)) + (az * az)), dr = sqrt(((bx * bx) + (by * by)) + (bz * bz));
        ok = fabs(ds - dr) <= thr;
      }
    }
    const u64 mask = __ballot(ok);
    if (lane == 0) adj[static_cast<size_t>(row) * W + w] = mask;
    deg += __popcll(mask);
  }
  if (lane == 0) degree[row] = deg;
}

// ---- (2) core numbers ----------------------------------------------------------------------------------------------------

// One block.  deg: working degrees, list: the vertices removed in the current round (both int32[C]).
__global__ __launch_bounds__(kOne) void core_kernel(const u64* __restrict__ adj, int C, int W, const int32_t* __restrict__ degree,
                                                    int32_t* __restrict__ core, int* __restrict__ deg, int* __restrict__ list,
                                                    RobustState* __restrict__ st) {
  __shared__ int s_cnt;
  __shared__ int s_red[kOne / kWave];
  int esum = 0;
  for (int i = threadIdx.x; i < C; i += kOne) {
    deg[i] = degree[i];
    core[i] = -1;
    esum += degree[i];
  }
  esum = wave_sum_i(esum);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = esum;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long e = 0;
    for (int w = 0; w < kOne / kWave; ++w) e += s_red[w];
    st->edges = static_cast<int>(e / 2);
  }
  int remaining = C, k = 0;
  while (remaining > 0) {  // every round removes a vertex or raises k, and k <= the largest degree < C
    __syncthreads();
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += kOne)
      if (core[i] < 0 && ld_agent(&deg[i]) <= k) {  // (the decrements are L2 atomics)
        core[i] = k;
        list[atomicAdd(&s_cnt, 1)] = i;  // at most C entries: a vertex is listed once
      }
    __syncthreads();
    const int n = s_cnt;
    if (n == 0) {
      ++k;
      continue;
    }
    remaining -= n;
    for (int q = threadIdx.x >> 6; q < n; q += kOne / kWave) {
      const int v = list[q];
      for (int w = threadIdx.x & 63; w < W; w += 64) {
        u64 bits = adj[static_cast<size_t>(v) * W + w];
        while (bits) {
          const int u = 64 * w + __builtin_ctzll(bits);
          bits &= bits - 1;
          if (core[u] < 0) atomicSub(&deg[u], 1);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) st->maxcore = C > 0 ? k : 0;  // the last level that removed a vertex
}

// ---- (3) maximum clique ----------------------------------------------------------------------------------------------------

// One block: greedy clique by (core number descending, row ascending) -> st->lb, greedy[0 .. lb); plans the search waves.
__global__ __launch_bounds__(kOne) void greedy_kernel(const u64* __restrict__ adj, int C, int W, const int32_t* __restrict__ core,
                                                      int* __restrict__ greedy, size_t pool_words, RobustState* __restrict__ st) {
  __shared__ u64 P[kMaxW];
  __shared__ u64 s_key[kOne / kWave];
  __shared__ int s_pick;
  for (int w = threadIdx.x; w < W; w += kOne) {
    const int left = C - 64 * w;
    P[w] = left >= 64 ? ~0ull : ((1ull << left) - 1);
  }
  __syncthreads();
  int size = 0;
  while (size < C) {  // a step adds a vertex or ends the loop
    u64 key = 0;      // (core + 1) << 32 | ~row: the highest core number, then the lowest row
    for (int u = threadIdx.x; u < C; u += kOne)
      if ((P[u >> 6] >> (u & 63)) & 1) {
        const u64 k2 = (static_cast<u64>(core[u] + 1) << 32) | static_cast<u64>(0xffffffffu - static_cast<unsigned>(u));
        key = k2 > key ? k2 : key;
      }
    key = wave_max_u64(key);
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 b = 0;
      for (int w = 0; w < kOne / kWave; ++w) b = s_key[w] > b ? s_key[w] : b;
      s_pick = b == 0 ? -1 : static_cast<int>(0xffffffffu - static_cast<unsigned>(b & 0xffffffffu));
    }
    __syncthreads();
    const int u = s_pick;
    if (u < 0) break;
    if (threadIdx.x == 0) greedy[size] = u;
    ++size;
    for (int w = threadIdx.x; w < W; w += kOne) P[w] &= adj[static_cast<size_t>(u) * W + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    st->lb = size;
    const int cap = st->maxcore + 2;  // a clique has at most max core + 1 rows
    st->depth_cap = cap;
    const size_t per_wave = static_cast<size_t>(cap) * (W + 1);
    size_t n = pool_words / per_wave;  // >= 1: the pool holds C + 2 levels
    st->n_waves = n > kSearchWaves ? kSearchWaves : static_cast<int>(n);
  }
}

// One wavefront per subproblem.  pool: per wave depth_cap levels of W words, then chosen[depth_cap] and best[depth_cap] (int32).
// wave_best: int32 [kSearchWaves, 2] = {size, v} of the wave's best subproblem (size 0: none).
__global__ __launch_bounds__(kBlock) void search_kernel(const u64* __restrict__ adj, int C, int W, const int32_t* __restrict__ core,
                                                        long long budget, u64* __restrict__ pool, int* __restrict__ wave_best,
                                                        RobustState* __restrict__ st) {
  const int g = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n_waves = st->n_waves, cap = st->depth_cap, need0 = st->lb;
  if (g >= n_waves) return;
  u64* stack = pool + static_cast<size_t>(g) * cap * (W + 1);
  int* chosen = reinterpret_cast<int*>(stack + static_cast<size_t>(cap) * W);
  int* best = chosen + cap;
  int best_size = 0, best_v = -1;
  bool exhausted = false;
  for (int v = g; v < C; v += n_waves) {
    if (core[v] < need0 - 1) continue;
    int cnt = 0;
    for (int w = lane; w < W; w += 64) {
      u64 bits = adj[static_cast<size_t>(v) * W + w];
      if (w < (v >> 6)) bits = 0;
      else if (w == (v >> 6)) bits &= ~((2ull << (v & 63)) - 1);  // rows above v only
      for (u64 b = bits; b; b &= b - 1) {
        const int u = 64 * w + __builtin_ctzll(b);
        if (core[u] < need0 - 1) bits &= ~(1ull << (u & 63));
      }
      stack[w] = bits;
      cnt += __popcll(bits);
    }
    cnt = wave_sum_i(cnt);
    if (1 + cnt < need0) continue;
    if (lane == 0) chosen[0] = v;
    int d = 0, need = need0;  // level d holds the untried candidates that extend chosen[0 .. d]
    long long nodes = 0;
    bool finished = false;
    while (nodes < budget) {
      ++nodes;
      u64* Pd = stack + static_cast<size_t>(d) * W;
      int c = 0, first = 0x7fffffff;
      for (int w = lane; w < W; w += 64) {
        const u64 bits = Pd[w];
        c += __popcll(bits);
        if (bits && first == 0x7fffffff) first = 64 * w + __builtin_ctzll(bits);
      }
      c = wave_sum_i(c);
      first = wave_min_i(first);
      const int cur = d + 1;
      if (cur + c >= need && c > 0) {
        if (d + 2 > cap) break;  // level d + 1 must exist (cliques have at most cap - 1 rows, so this does not happen)
        if (lane == (first >> 6) % 64) Pd[first >> 6] &= ~(1ull << (first & 63));
        if (lane == 0) chosen[d + 1] = first;
        u64* Pn = Pd + W;
        for (int w = lane; w < W; w += 64) Pn[w] = Pd[w] & adj[static_cast<size_t>(first) * W + w];
        ++d;
        continue;
      }
      if (cur + c >= need) {  // c == 0: a maximal clique of an accepted size
        need = cur + 1;
        if (cur > best_size) {
          best_size = cur;
          best_v = v;
          if (lane == 0)
            for (int q = 0; q < cur; ++q) best[q] = chosen[q];
        }
      }
      if (d == 0) {
        finished = true;
        break;
      }
      --d;
    }
    if (!finished) exhausted = true;
  }
  if (lane == 0) {
    wave_best[2 * g] = best_size;
    wave_best[2 * g + 1] = best_v;
    if (exhausted) atomicOr(&st->exhausted, 1);
  }
}

// One block: the selected rows as an ascending list.  mode as RDM_ROBUST_*.
__global__ __launch_bounds__(kOne) void select_kernel(int mode, int C, int W, const int32_t* __restrict__ core,
                                                      const int* __restrict__ greedy, const u64* __restrict__ pool,
                                                      const int* __restrict__ wave_best, int32_t* __restrict__ selected,
                                                      RobustState* __restrict__ st) {
  __shared__ u64 S[kMaxW];
  __shared__ int s_off[kMaxW + 1];
  __shared__ int s_src, s_size;
  for (int w = threadIdx.x; w < kMaxW; w += kOne) S[w] = 0;
  __syncthreads();
  if (mode == RDM_ROBUST_CLIQUE) {
    if (threadIdx.x == 0) {
      int bs = 0, bv = 0x7fffffff, bg = -1;
      for (int g = 0; g < st->n_waves; ++g) {
        const int s = wave_best[2 * g], v = wave_best[2 * g + 1];
        if (s > bs || (s == bs && s > 0 && v < bv)) {
          bs = s; bv = v; bg = g;
        }
      }
      if (bs < st->lb) bg = -1;  // nothing accepted before the budgets ran out: the greedy clique
      s_src = bg;
      s_size = bg >= 0 ? bs : st->lb;
    }
    __syncthreads();
    const int cap = st->depth_cap;
    const int* rows = greedy;
    if (s_src >= 0) {
      const u64* stack = pool + static_cast<size_t>(s_src) * cap * (W + 1);
      rows = reinterpret_cast<const int*>(stack + static_cast<size_t>(cap) * W) + cap;
    }
    if (threadIdx.x == 0)
      for (int q = 0; q < s_size; ++q) {
        const int u = rows[q];
        if (u >= 0 && u < C) S[u >> 6] |= 1ull << (u & 63);
      }
  } else {
    const int mc = st->maxcore;
    for (int w = threadIdx.x; w < W; w += kOne) {
      u64 bits = 0;
      for (int b = 0; b < 64; ++b) {
        const int u = 64 * w + b;
        if (u < C && (mode == RDM_ROBUST_NONE || core[u] == mc)) bits |= 1ull << b;
      }
      S[w] = bits;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int off = 0;
    for (int w = 0; w < W; ++w) {
      s_off[w] = off;
      off += __popcll(S[w]);
    }
    s_off[W] = off;
    st->K = off;
    st->unit_weights = 1;
    st->valid = off >= 3 ? 1 : 0;
    if (off < 3) st->done = 1;
  }
  __syncthreads();
  for (int w = threadIdx.x; w < W; w += kOne) {
    int o = s_off[w];
    for (u64 b = S[w]; b; b &= b - 1) selected[o++] = 64 * w + __builtin_ctzll(b);
  }
  for (int i = s_off[W] + threadIdx.x; i < C; i += kOne) selected[i] = -1;
}

// ---- (4) GNC-TLS rotation ----------------------------------------------------------------------------------------------------

struct Pair {
  double a[3], b[3];
};
__device__ __forceinline__ Pair load_pair(const float* __restrict__ src, const float* __restrict__ ref, int ip, int iq) {
  Pair m;
  for (int k = 0; k < 3; ++k) {
    m.a[k] = static_cast<double>(src[3 * iq + k]) - static_cast<double>(src[3 * ip + k]);
    m.b[k] = static_cast<double>(ref[3 * iq + k]) - static_cast<double>(ref[3 * ip + k]);
  }
  return m;
}
__device__ __forceinline__ double residual2(const double* R, const Pair& m) {
  const double dx = m.b[0] - ((R[0] * m.a[0] + R[1] * m.a[1]) + R[2] * m.a[2]);
  const double dy = m.b[1] - ((R[3] * m.a[0] + R[4] * m.a[1]) + R[5] * m.a[2]);
  const double dz = m.b[2] - ((R[6] * m.a[0] + R[7] * m.a[1]) + R[8] * m.a[2]);
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}
// The weight the last decision gave a pair (n2: squared noise bound).
__device__ __forceinline__ double weight_of(const RobustState& s, double n2, const Pair& m) {
  if (s.unit_weights) return 1.0;
  const double r2 = residual2(s.Rw, m);
  if (r2 >= s.th1) return 0.0;
  if (r2 <= s.th2) return 1.0;
  return sqrt(((n2 * s.muw) * (s.muw + 1.0)) / r2) - s.muw;
}

// H[a][b] = sum w a_a b_b over the pairs: block x takes p = x, x + gridDim, ..., its threads q = p + 1 + t, ... -> slab[block][9]
__global__ __launch_bounds__(kBlock) void gnc_sum_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                         const int32_t* __restrict__ sel, double n2,
                                                         const RobustState* __restrict__ st, double* __restrict__ slab) {
  if (st->done) return;
  const RobustState s = *st;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = blockIdx.x; p < s.K; p += gridDim.x) {
    const int ip = sel[p];
    for (int q = p + 1 + threadIdx.x; q < s.K; q += kBlock) {
      const Pair m = load_pair(src, ref, ip, sel[q]);
      const double w = weight_of(s, n2, m);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[3 * a + b] += (w * m.a[a]) * m.b[b];
    }
  }
  const double sum = block_sum<9, kBlock>(acc, threadIdx.x);
  if (threadIdx.x < 9) slab[blockIdx.x * 9 + threadIdx.x] = sum;
}

// One thread: the slabs in order -> Horn's rotation.
__global__ void gnc_solve_kernel(const double* __restrict__ slab, int rows, RobustState* __restrict__ st) {
  if (st->done || threadIdx.x != 0) return;
  double H[9];
  for (int k = 0; k < 9; ++k) {
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += slab[r * 9 + k];
    H[k] = s;
  }
  double R[9];
  kabsch_rotation(H, R);
  for (int k = 0; k < 9; ++k) st->R[k] = R[k];
}

// cost = sum w r2 (old weights, new rotation) and max r2 -> slab[block][2]
__global__ __launch_bounds__(kBlock) void gnc_residual_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                              const int32_t* __restrict__ sel, double n2,
                                                              const RobustState* __restrict__ st, double* __restrict__ slab) {
  if (st->done) return;
  const RobustState s = *st;
  double acc[1] = {0};
  double mx = 0.0;
  for (int p = blockIdx.x; p < s.K; p += gridDim.x) {
    const int ip = sel[p];
    for (int q = p + 1 + threadIdx.x; q < s.K; q += kBlock) {
      const Pair m = load_pair(src, ref, ip, sel[q]);
      const double r2 = residual2(s.R, m);
      acc[0] += weight_of(s, n2, m) * r2;
      mx = r2 > mx ? r2 : mx;
    }
  }
  __shared__ double s_mx[kBlock / kWave];
  mx = wave_max_d(mx);
  if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
  const double cost = block_sum<1, kBlock>(acc, threadIdx.x);  // (synchronises)
  if (threadIdx.x == 0) {
    slab[blockIdx.x * 2] = cost;
    double m2 = s_mx[0];
    for (int w = 1; w < kBlock / kWave; ++w) m2 = s_mx[w] > m2 ? s_mx[w] : m2;
    slab[blockIdx.x * 2 + 1] = m2;
  }
}

// One thread, iteration `it`: thresholds, the new weights' definition, the stopping rule.
__global__ void gnc_decide_kernel(const double* __restrict__ slab, int rows, int it, int max_iterations, double n2, double gnc_factor,
                                  double cost_threshold, RobustState* __restrict__ st) {
  if (st->done || threadIdx.x != 0) return;
  double cost = 0.0, mx = 0.0;
  for (int r = 0; r < rows; ++r) {
    cost += slab[2 * r];
    mx = slab[2 * r + 1] > mx ? slab[2 * r + 1] : mx;
  }
  st->iterations = it + 1;
  if (it == 0) {
    st->mu = 1.0 / ((2.0 * mx) / n2 - 1.0);
    if (st->mu <= 0.0) {  // every pair is an inlier: the weights stay 1
      st->done = 1;
      return;
    }
  }
  const double mu = st->mu;
  st->th1 = ((mu + 1.0) / mu) * n2;
  st->th2 = (mu / (mu + 1.0)) * n2;
  st->muw = mu;
  for (int k = 0; k < 9; ++k) st->Rw[k] = st->R[k];
  st->unit_weights = 0;
  if ((it > 0 && fabs(cost - st->prev_cost) < cost_threshold) || it + 1 >= max_iterations) st->done = 1;
  st->prev_cost = cost;
  st->mu = mu * gnc_factor;
}

__global__ __launch_bounds__(kBlock) void weights_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                         const int32_t* __restrict__ sel, double n2,
                                                         const RobustState* __restrict__ st, double* __restrict__ weights,
                                                         long long capacity) {
  const RobustState s = *st;
  if (!s.valid) return;
  for (int p = blockIdx.x; p < s.K; p += gridDim.x) {
    const int ip = sel[p];
    const long long base = static_cast<long long>(p) * s.K - static_cast<long long>(p) * (p + 1) / 2 - p - 1;
    for (int q = p + 1 + threadIdx.x; q < s.K; q += kBlock) {
      const long long e = base + q;
      if (e < capacity) weights[e] = weight_of(s, n2, load_pair(src, ref, ip, sel[q]));
    }
  }
}

// ---- (5) translation ----------------------------------------------------------------------------------------------------------

// x[axis][k] (stride C) and the interval ends h[axis][2k], h[axis][2k + 1] (stride 2C)
__global__ __launch_bounds__(kBlock) void trans_values_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                              const int32_t* __restrict__ sel, int C, double c,
                                                              const RobustState* __restrict__ st, double* __restrict__ x,
                                                              double* __restrict__ h) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (!st->valid || k >= st->K) return;
  const int i = sel[k];
  const double sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
  for (int a = 0; a < 3; ++a) {
    const double* R = st->R + 3 * a;
    const double v = static_cast<double>(ref[3 * i + a]) - ((R[0] * sx + R[1] * sy) + R[2] * sz);
    x[static_cast<size_t>(a) * C + k] = v;
    h[static_cast<size_t>(a) * 2 * C + 2 * k] = v - c;
    h[static_cast<size_t>(a) * 2 * C + 2 * k + 1] = v + c;
  }
}

// hs[axis][rank of h[axis][i]] = h[axis][i]; rank = values below it, or equal with a lower position (always < 2K)
__global__ __launch_bounds__(kBlock) void trans_rank_kernel(int C, const RobustState* __restrict__ st, const double* __restrict__ h,
                                                            double* __restrict__ hs) {
  const int i = blockIdx.x * kBlock + threadIdx.x, a = blockIdx.y;
  if (!st->valid || i >= 2 * st->K) return;
  const double* ha = h + static_cast<size_t>(a) * 2 * C;
  const double v = ha[i];
  const int n = 2 * st->K;
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const double u = ha[j];
    rank += (u < v || (u == v && j < i)) ? 1 : 0;
  }
  hs[static_cast<size_t>(a) * 2 * C + rank] = v;
}

// one thread per midpoint: consensus set, its mean and cost (sums over k ascending)
__global__ __launch_bounds__(kBlock) void trans_cost_kernel(int C, double c, const RobustState* __restrict__ st,
                                                            const double* __restrict__ x, const double* __restrict__ hs,
                                                            double* __restrict__ cost, double* __restrict__ est) {
  const int i = blockIdx.x * kBlock + threadIdx.x, a = blockIdx.y;
  if (!st->valid || i >= 2 * st->K - 1) return;
  const int K = st->K;
  const double* xa = x + static_cast<size_t>(a) * C;
  const double* ha = hs + static_cast<size_t>(a) * 2 * C;
  const double m = (ha[i] + ha[i + 1]) * 0.5;
  double sum = 0.0;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    const double v = xa[k];
    if (fabs(v - m) <= c) {
      sum += v;
      ++n;
    }
  }
  double e = 0.0, cs = INFINITY;
  if (n > 0) {
    e = sum / static_cast<double>(n);
    double s2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const double v = xa[k];
      if (fabs(v - m) <= c) s2 += (v - e) * (v - e);
    }
    cs = s2 + static_cast<double>(K - n) * (c * c);
  }
  cost[static_cast<size_t>(a) * 2 * C + i] = cs;
  est[static_cast<size_t>(a) * 2 * C + i] = e;
}

// One block: per axis the est of least cost (lowest midpoint among equals), the inlier count, the outputs.
__global__ __launch_bounds__(kOne) void finish_kernel(int C, double c, RobustState* __restrict__ st, const double* __restrict__ x,
                                                      const double* __restrict__ cost, const double* __restrict__ est,
                                                      double* __restrict__ transform, int32_t* __restrict__ stats) {
  __shared__ double s_c[kOne];
  __shared__ int s_i[kOne];
  __shared__ double s_t[3];
  const int K = st->K, valid = st->valid;
  int inl = 0;
  if (valid) {
    for (int a = 0; a < 3; ++a) {
      const double* ca = cost + static_cast<size_t>(a) * 2 * C;
      double bc = INFINITY;
      int bi = 0x7fffffff;
      for (int i = threadIdx.x; i < 2 * K - 1; i += kOne) {
        const double v = ca[i];
        if (v < bc) {  // ascending i per thread: equals keep the lower midpoint
          bc = v; bi = i;
        }
      }
      s_c[threadIdx.x] = bc;
      s_i[threadIdx.x] = bi;
      __syncthreads();
      for (int o = kOne / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
          const double c2 = s_c[threadIdx.x + o], c1 = s_c[threadIdx.x];
          const int i2 = s_i[threadIdx.x + o], i1 = s_i[threadIdx.x];
          if (c2 < c1 || (c2 == c1 && i2 < i1)) {
            s_c[threadIdx.x] = c2; s_i[threadIdx.x] = i2;
          }
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) s_t[a] = s_i[0] < 2 * K - 1 ? est[static_cast<size_t>(a) * 2 * C + s_i[0]] : 0.0;
      __syncthreads();
    }
    for (int k = threadIdx.x; k < K; k += kOne) {
      bool ok = true;
      for (int a = 0; a < 3; ++a) ok = ok && fabs(x[static_cast<size_t>(a) * C + k] - s_t[a]) <= c;
      inl += ok ? 1 : 0;
    }
  }
  inl = wave_sum_i(inl);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_i[threadIdx.x >> 6] = inl;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kOne / kWave; ++w) total += s_i[w];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) transform[4 * a + b] = valid ? st->R[3 * a + b] : (a == b ? 1.0 : 0.0);
      transform[4 * a + 3] = valid ? s_t[a] : 0.0;
      transform[12 + a] = 0.0;
    }
    transform[15] = 1.0;
    stats[0] = K;
    stats[1] = valid;
    stats[2] = st->exhausted ? 0 : 1;
    stats[3] = valid ? st->iterations : 0;
    stats[4] = total;
    stats[5] = st->edges;
  }
}

__global__ void empty_kernel(double* __restrict__ transform, int32_t* __restrict__ stats) {
  const int t = threadIdx.x;
  if (t < 16) transform[t] = (t % 5 == 0) ? 1.0 : 0.0;
  if (t < RDM_ROBUST_STATS) stats[t] = t == 2 ? 1 : 0;
}

// ---- host --------------------------------------------------------------------------------------------------------------------

struct Work {
  RobustState* st;
  u64* adj;
  int32_t *degree, *core;
  int *deg, *list, *greedy, *wave_best;
  u64* pool;
  size_t pool_words;
  double *slab_h, *slab_c, *x, *h, *hs, *cost, *est;
};

bool carve(Arena& ar, int64_t C, int mode, Work& w) {
  const size_t n = static_cast<size_t>(C > 0 ? C : 1), W = (n + 63) / 64;
  w.st = ar.take<RobustState>(1);
  w.adj = ar.take<u64>(n * W);
  w.degree = ar.take<int32_t>(n);
  w.core = ar.take<int32_t>(n);
  w.deg = ar.take<int>(n);
  w.list = ar.take<int>(n);
  w.greedy = ar.take<int>(n);
  w.wave_best = ar.take<int>(2 * kSearchWaves);
  const size_t one = (n + 2) * (W + 1);  // a wave's stack at the largest depth cap
  size_t waves = kPoolBytes / (one * sizeof(u64));
  waves = waves < 1 ? 1 : (waves > kSearchWaves ? kSearchWaves : waves);
  w.pool_words = mode == RDM_ROBUST_CLIQUE ? one * waves : 1;
  w.pool = ar.take<u64>(w.pool_words);
  w.slab_h = ar.take<double>(kPairBlocks * 9);
  w.slab_c = ar.take<double>(kPairBlocks * 2);
  w.x = ar.take<double>(3 * n);
  w.h = ar.take<double>(6 * n);
  w.hs = ar.take<double>(6 * n);
  w.cost = ar.take<double>(6 * n);
  w.est = ar.take<double>(6 * n);
  return ar.ok;
}

}  // namespace

extern "C" int64_t rdm_robust_default_clique_nodes(void) { return kDefaultCliqueNodes; }

extern "C" size_t rdm_robust_registration_workspace_bytes(int64_t n_corr, int inlier_selection) {
  using namespace rdm;
  if (n_corr < 0 || n_corr > RDM_ROBUST_MAX_CORR) return 0;
  Arena ar(nullptr, 0);
  Work w;
  carve(ar, n_corr, inlier_selection, w);
  return ar.off;
}

extern "C" int rdm_robust_registration(const float* src_corr, const float* ref_corr, int64_t n_corr, double noise_bound, double cbar2,
                                       double gnc_factor, int max_iterations, double cost_threshold, int inlier_selection,
                                       int64_t max_clique_nodes, double* transform, int32_t* stats, int32_t* selected,
                                       double* weights, int64_t weights_capacity, int32_t* degree, int32_t* core, void* ws,
                                       size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(transform && stats, "rdm_robust_registration: null output");
  RDM_REQUIRE(n_corr >= 0 && noise_bound > 0.0 && std::isfinite(noise_bound) && cbar2 > 0.0 && std::isfinite(cbar2) &&
                  gnc_factor > 1.0 && std::isfinite(gnc_factor) && max_iterations >= 1 && cost_threshold >= 0.0 &&
                  inlier_selection >= RDM_ROBUST_CLIQUE && inlier_selection <= RDM_ROBUST_NONE && weights_capacity >= 0,
              "rdm_robust_registration: bad arguments");
  if (n_corr > RDM_ROBUST_MAX_CORR) {
    set_error("rdm_robust_registration: %lld correspondences, the compatibility graph holds at most %d",
              static_cast<long long>(n_corr), RDM_ROBUST_MAX_CORR);
    return RDM_ERR_CAPACITY;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_corr == 0) {
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, s, transform, stats);
    return launch_status("rdm_robust_registration");
  }
  RDM_REQUIRE(src_corr && ref_corr && selected, "rdm_robust_registration: null correspondences or selection");
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, n_corr, inlier_selection, w)) {
    set_error("rdm_robust_registration: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  if (degree) w.degree = degree;
  if (core) w.core = core;
  const int C = static_cast<int>(n_corr), W = (C + 63) / 64;
  const double root = sqrt(cbar2), thr = (2.0 * noise_bound) * root, c = noise_bound * root;
  const double n2 = ((2.0 * noise_bound) * (2.0 * noise_bound)) * cbar2;
  const long long budget = max_clique_nodes > 0 ? max_clique_nodes : kDefaultCliqueNodes;
  RDM_HIP_CHECK(hipMemsetAsync(w.st, 0, sizeof(RobustState), s));
  hipLaunchKernelGGL(graph_kernel, dim3(ceil_div(C, kBlock / kWave)), dim3(kBlock), 0, s, src_corr, ref_corr, C, W, thr, w.adj,
                     w.degree);
  hipLaunchKernelGGL(core_kernel, dim3(1), dim3(kOne), 0, s, w.adj, C, W, w.degree, w.core, w.deg, w.list, w.st);
  if (inlier_selection == RDM_ROBUST_CLIQUE) {
    hipLaunchKernelGGL(greedy_kernel, dim3(1), dim3(kOne), 0, s, w.adj, C, W, w.core, w.greedy, w.pool_words, w.st);
    hipLaunchKernelGGL(search_kernel, dim3(kSearchWaves / (kBlock / kWave)), dim3(kBlock), 0, s, w.adj, C, W, w.core, budget, w.pool,
                       w.wave_best, w.st);
  }
  hipLaunchKernelGGL(select_kernel, dim3(1), dim3(kOne), 0, s, inlier_selection, C, W, w.core, w.greedy, w.pool, w.wave_best, selected,
                     w.st);
  int rc = launch_status("rdm_robust_registration (selection)");
  if (rc != RDM_OK) return rc;
  const int pb = C < kPairBlocks ? C : kPairBlocks;
  int done = 0;
  for (int it = 0; it < max_iterations && done == 0;) {
    const int end = max_iterations - it < kChunk ? max_iterations : it + kChunk;
    for (; it < end; ++it) {
      hipLaunchKernelGGL(gnc_sum_kernel, dim3(pb), dim3(kBlock), 0, s, src_corr, ref_corr, selected, n2, w.st, w.slab_h);
      hipLaunchKernelGGL(gnc_solve_kernel, dim3(1), dim3(64), 0, s, w.slab_h, pb, w.st);
      hipLaunchKernelGGL(gnc_residual_kernel, dim3(pb), dim3(kBlock), 0, s, src_corr, ref_corr, selected, n2, w.st, w.slab_c);
      hipLaunchKernelGGL(gnc_decide_kernel, dim3(1), dim3(64), 0, s, w.slab_c, pb, it, max_iterations, n2, gnc_factor, cost_threshold,
                         w.st);
    }
    rc = launch_status("rdm_robust_registration (rotation)");
    if (rc != RDM_OK) return rc;
    RDM_HIP_CHECK(hipMemcpyAsync(&done, &w.st->done, sizeof(int), hipMemcpyDeviceToHost, s));  // one 4-byte read-back per chunk
    RDM_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (weights && weights_capacity > 0)
    hipLaunchKernelGGL(weights_kernel, dim3(pb), dim3(kBlock), 0, s, src_corr, ref_corr, selected, n2, w.st, weights,
                       static_cast<long long>(weights_capacity));
  const dim3 gk(ceil_div(C, kBlock)), g2(ceil_div(2 * C, kBlock), 3);
  hipLaunchKernelGGL(trans_values_kernel, gk, dim3(kBlock), 0, s, src_corr, ref_corr, selected, C, c, w.st, w.x, w.h);
  hipLaunchKernelGGL(trans_rank_kernel, g2, dim3(kBlock), 0, s, C, w.st, w.h, w.hs);
  hipLaunchKernelGGL(trans_cost_kernel, g2, dim3(kBlock), 0, s, C, c, w.st, w.x, w.hs, w.cost, w.est);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kOne), 0, s, C, c, w.st, w.x, w.cost, w.est, transform, stats);
  return launch_status("rdm_robust_registration");
}
