// Exact cloud-to-cloud nearest neighbours: get_nearest_neighbor (geotransformer/utils/pointcloud.py:11-22, a cKDTree k = 1
// query) and what the reference builds on it -- compute_overlap, compute_modified_chamfer_distance, compute_registration_rmse
// (geotransformer/utils/registration.py:136-197) -- plus the fitness / inlier RMSE of a pose.
//
// Definition, to the bit (x', d2 and ties: cell_index.h; tests/nearest_restatement.py is the float64 numpy restatement):
//   q [n_q, >=3] / s [n_s, >=3]; each cloud has an optional transform;  d = q' - s' per axis;
//   d2[i] = the smallest d2 over ALL support rows, idx[i] = the LOWEST support row that attains it (cKDTree leaves equal
//   distances open; this library defines the tie);  the distance is sqrt(d2) in double;  n_s = 0 gives d2 = +inf, idx = n_s.
//
// Structure:
//   move: q' and s' as float64 [n, 3] (the identity copies); per-block slabs of the coordinate box and a non-finite flag.
//   setup (one thread): the cell edge h -- the caller's, or (cell <= 0) the edge of a cube that holds about 8 support points at
//   uniform density over the box, raised so that the box stays under cell_index.h's limits -- and the cell box of s'.
//   index: cell_index.h over s'.
//   phase 1 (nn_shell_kernel), one wavefront per query row: the 3 x 3 cell columns around the query's cell (lanes bisect one
//   column each, the wave walks the ranges 64 records at a time), then the 5 x 5 columns; smallest (d2, j) by wave butterfly.
//   The row is SETTLED when d2 < reach^2, reach = the distance from the query to the nearest face of the cube of cells searched
//   so far, computed in double and rounded towards the query by a 2^-48 relative margin -- 32 times the rounding of floor(x / h)
//   and of d2 -- so every support point outside the cube has a strictly larger COMPUTED d2.  A query outside the box of s' is
//   never settled here.
//   list: an ordered (stable) compaction of the unsettled rows; its length stays on the device until the call's read-back.
//   phase 2 (nn_sweep_kernel), 64 unsettled rows per workgroup, one per lane: every support row, staged through LDS in tiles of
//   1024 and read as broadcasts, each wavefront a quarter of the tile in ascending j with a strict comparison; the four
//   partials merge by (d2, j).
//   reduce: sum of sqrt(d2), rows with sqrt(d2) < radius (strict) and their sum of d2: float64, per thread in row order, lanes
//   by butterfly, wavefronts and block slabs in order; the launch geometry depends on n_q only.
// Both phases evaluate the same expression on the same doubles and order candidates by (d2, j), so the result does not depend
// on h, on the path a row takes or on scheduling: no float atomics, two calls give the same bits.
// A point that is not finite, before or after moving, or a support point beyond the cell limits, sets the status before
// anything is indexed: every later kernel returns at once, the outputs stay untouched and the call returns RDM_ERR_ARG.
//
// rdm_information_matrix (Open3D's get_information_matrix_from_point_clouds / evaluate_registration; parity unpinned, pinned to
// tests/information_restatement.py) runs the phases above once, q = source, s = target, and then, over the rows with
// sqrt(d2) < radius (STRICT: the rows the reduce step counts; Open3D's own comparison is library-internal, this library defines
// it), p = s'_idx the MOVED TARGET point: the sum of g g^T for g = (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1)
// in closed form -- C = sum 1 (an integer), sum p, sum p p^T: rotation block tr(M) I - M, translation block C I, upper-right
// block [sum p]x, its transpose below -- with the reduce step's sums (info_sum_kernel, info_totals_kernel); optionally the rows
// (i, idx[i]) in ascending i by a second ordered compaction (info_corr_kernel; no atomic counter); one read-back of 40 doubles.
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "../../include/rdmnet_hip.h"
#include "common.h"

#pragma clang fp contract(off)

#include "cell_index.h"

namespace {
using namespace rdm;

constexpr int kBlock = kCellBlock;
constexpr int kRowsPerBlock = kBlock / kWave;  // phase 1: query rows (wavefronts) per workgroup
constexpr int kRings = 2;                      // phase 1 searches cubes of 3^3, then 5^3 cells
constexpr int kTile = 1024;                    // phase 2: support rows per LDS tile
constexpr int kSweepMaxBlocks = 8192;
constexpr double kMargin = 3.5527136788005009e-15;  // 2^-48

struct NnState {
  int stop;         // 2: a point that is not finite, or a support point beyond the cell limits
  unsigned n_list;  // unsettled rows (written by the compaction)
  unsigned n_corr;  // rdm_information_matrix: rows under the radius (written by its compaction)
  double radius;
};

// Per block: lowest and highest coordinate per axis and a bad flag (a non-finite coordinate) -> slab[block][8].
__global__ __launch_bounds__(kBlock) void nn_box_kernel(const double* __restrict__ moved, int n, double* __restrict__ slab) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
  for (long long j = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; j < n; j += static_cast<long long>(gridDim.x) * kBlock) {
    for (int a = 0; a < 3; ++a) {
      const double v = moved[3 * j + a];
      if (!isfinite(v)) bad = 1.0;
      lo[a] = fmin(lo[a], v);
      hi[a] = fmax(hi[a], v);
    }
  }
  block_box(lo, hi, bad, slab);
}

// One thread: the status of a new call, the cell edge and the cell box of the moved support cloud.
__global__ void nn_setup_kernel(const double* __restrict__ slab_s, int rows_s, int m, const double* __restrict__ slab_q, int rows_q,
                                double cell, double radius, Grid* __restrict__ grid, NnState* __restrict__ st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (int r = 0; r < rows_s; ++r) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], slab_s[r * 8 + a]);
      hi[a] = fmax(hi[a], slab_s[r * 8 + 3 + a]);
    }
    bad = bad || slab_s[r * 8 + 6] != 0.0;
  }
  for (int r = 0; r < rows_q; ++r) bad = bad || slab_q[r * 8 + 6] != 0.0;
  double h = cell > 0.0 ? cell : 1.0;
  long long glo[3] = {0, 0, 0}, gdims[3] = {0, 0, 0};
  if (m > 0 && !bad) {
    if (!(cell > 0.0)) {  // about 8 points per cell at uniform density over the box (a flat box counts 1/1024 of its widest side)
      double widest = 0.0, reach = 0.0;
      for (int a = 0; a < 3; ++a) {
        widest = fmax(widest, hi[a] - lo[a]);
        reach = fmax(reach, fmax(fabs(lo[a]), fabs(hi[a])));
      }
      double volume = 1.0;
      for (int a = 0; a < 3; ++a) volume *= fmax(hi[a] - lo[a], widest * (1.0 / 1024.0));
      h = cbrt(8.0 * volume / static_cast<double>(m));
      h = fmax(h, fmax(reach * (1.0 / 536870912.0), widest * (1.0 / 1048576.0)));  // |p / h| <= 2^29, at most 2^20 + 1 cells per axis
      if (!(h > 0.0) || !isfinite(h)) h = 1.0;                                       // (one point, or all points equal)
    }
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {  // floor(x / h) does not decrease with x: the cells of the lowest and highest coordinate bound all
      const double c0 = cell_of(lo[a], h), c1 = cell_of(hi[a], h);
      if (!(fabs(c0) < kCellLimit && fabs(c1) < kCellLimit)) {
        bad = true;
        break;
      }
      glo[a] = static_cast<long long>(c0);
      gdims[a] = static_cast<long long>(c1 - c0 + 1.0);
      cells *= c1 - c0 + 1.0;
    }
    if (cells > 4611686018427387904.0) bad = true;  // keys are 64-bit: the box must fit 2^62 cells
  }
  for (int a = 0; a < 3; ++a) {
    grid->lo[a] = bad ? 0 : glo[a];
    grid->dims[a] = bad ? 0 : gdims[a];
  }
  grid->h = h;
  st->stop = bad ? 2 : 0;
  st->n_list = 0;
  st->n_corr = 0;
  st->radius = radius;
}

// the smaller of two candidates by (d2, row)
__device__ __forceinline__ void take(double& bd, int& bi, double d, int i) {
  if (d < bd || (d == bd && i < bi)) {
    bd = d;
    bi = i;
  }
}

// Phase 1: one wavefront per query row.
__global__ __launch_bounds__(kBlock) void nn_shell_kernel(const double* __restrict__ qm, int n, const unsigned long long* __restrict__ keys,
                                                          const Rec* __restrict__ recs, int m, const Grid* __restrict__ grid,
                                                          const NnState* __restrict__ st, int* __restrict__ idx,
                                                          double* __restrict__ d2, uint8_t* __restrict__ open) {
  const int lane = lane_id();
  const long long i = static_cast<long long>(blockIdx.x) * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= n || st->stop != 0) return;  // (wave-uniform)
  double bd = INFINITY;
  int bi = m;
  bool settled = m == 0;  // (nothing to sweep either)
  if (m > 0) {
    const Grid g = *grid;
    const double q[3] = {qm[3 * i], qm[3 * i + 1], qm[3 * i + 2]};
    long long c[3] = {0, 0, 0};
    const bool inside = query_cell(q, g, 0, c);
    for (int rho = 1; rho <= kRings && inside && !settled; ++rho) {  // (wave-uniform)
      const int w = 2 * rho + 1;
      int begin = 0, end = 0;
      if (lane < w * w) {  // lane -> one cell column (x-major, so ascending keys)
        const long long x = c[0] - rho + lane / w, y = c[1] - rho + lane % w;
        long long z0, z1;
        ring_heights(g, c[2], rho, &z0, &z1);  // (never empty: the query's cell is inside)
        if (x >= 0 && x < g.dims[0] && y >= 0 && y < g.dims[1]) {
          unsigned long long klo, khi;
          column_keys(g, x, y, z0, z1, &klo, &khi);
          begin = lower_bound(keys, m, klo);
          end = lower_bound(keys, m, khi + 1);
        }
      }
      for (int cc = 0; cc < w * w; ++cc) {
        const int b = __shfl(begin, cc, 64), e = __shfl(end, cc, 64);
        for (int p0 = b; p0 < e; p0 += kWave) {  // (wave-uniform bounds)
          const int p = p0 + lane;
          if (p < e) {
            const Rec s = recs[p];
            take(bd, bi, sq_dist(q[0], q[1], q[2], s.x, s.y, s.z), static_cast<int>(s.j));
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        take(bd, bi, od, oi);
      }
      // the distance to the nearest face of the cube of cells [c - rho, c + rho], rounded towards the query
      double reach = INFINITY;
      for (int a = 0; a < 3; ++a) {
        const double below = static_cast<double>(g.lo[a] + c[a] - rho) * g.h, above = static_cast<double>(g.lo[a] + c[a] + rho + 1) * g.h;
        const double margin = kMargin * fmax(fmax(fabs(below), fabs(above)), fabs(q[a]));
        reach = fmin(reach, fmin((q[a] - below) - margin, (above - q[a]) - margin));
      }
      reach = reach * (1.0 - kMargin);
      settled = reach > 0.0 && bd < reach * reach;
    }
  }
  if (lane == 0) {
    idx[i] = bi;
    d2[i] = bd;
    open[i] = settled ? 0 : 1;
  }
}

// Phase 2: 64 unsettled rows per workgroup (row = lane), every support row through LDS.
__global__ __launch_bounds__(kBlock) void nn_sweep_kernel(const double* __restrict__ qm, const double* __restrict__ sm, int m,
                                                          const int* __restrict__ list, const NnState* __restrict__ st,
                                                          int* __restrict__ idx, double* __restrict__ d2) {
  if (st->stop != 0) return;
  __shared__ double tile[3 * kTile];
  __shared__ double part_d[kRowsPerBlock][kWave];
  __shared__ int part_i[kRowsPerBlock][kWave];
  const long long count = st->n_list;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  constexpr int kPer = kTile / kRowsPerBlock;  // support rows of a tile per wavefront
  for (long long g0 = static_cast<long long>(blockIdx.x) * kWave; g0 < count; g0 += static_cast<long long>(gridDim.x) * kWave) {  // (block-uniform)
    const bool live = g0 + lane < count;
    const long long row = live ? list[g0 + lane] : 0;
    const double qx = live ? qm[3 * row] : 0.0, qy = live ? qm[3 * row + 1] : 0.0, qz = live ? qm[3 * row + 2] : 0.0;
    double bd = INFINITY;
    int bi = m;
    for (long long j0 = 0; j0 < m; j0 += kTile) {
      const int len = m - j0 < kTile ? static_cast<int>(m - j0) : kTile;
      __syncthreads();  // (the tile of the step before is read out)
      for (int k = threadIdx.x; k < 3 * len; k += kBlock) tile[k] = sm[3 * j0 + k];
      __syncthreads();
      const int k1 = len < (wave + 1) * kPer ? len : (wave + 1) * kPer;
      for (int k = wave * kPer; k < k1; ++k) {  // ascending j, strict: the lowest row among equal d2
        const double d = sq_dist(qx, qy, qz, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]);
        if (d < bd) {
          bd = d;
          bi = static_cast<int>(j0 + k);
        }
      }
    }
    part_d[wave][lane] = bd;
    part_i[wave][lane] = bi;
    __syncthreads();
    if (wave == 0) {
      for (int w = 1; w < kRowsPerBlock; ++w) take(bd, bi, part_d[w][lane], part_i[w][lane]);
      if (live) {
        idx[row] = bi;
        d2[row] = bd;
      }
    }
    __syncthreads();  // (the partials are read out)
  }
}

// Block sums of three float64 terms in a fixed order (common.h: block_sum) -> slab[block][4]
__device__ __forceinline__ void block_sums(double a, double b, double c, double* __restrict__ slab) {
  double v[3] = {a, b, c};
  const double s = block_sum<3, kBlock>(v, threadIdx.x);
  if (threadIdx.x < 3) slab[blockIdx.x * 4 + threadIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void nn_sum_kernel(const double* __restrict__ d2, int n, const NnState* __restrict__ st,
                                                        double* __restrict__ slab) {
  if (st->stop != 0) return;
  const double r = st->radius;
  double sum_dist = 0.0, within = 0.0, sum_d2 = 0.0;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kBlock) {
    const double v = d2[i], d = sqrt(v);
    sum_dist += d;
    if (d < r) {  // (strict, as compute_overlap; never with radius <= 0)
      within += 1.0;
      sum_d2 += v;
    }
  }
  block_sums(sum_dist, within, sum_d2, slab);
}

// One thread: {sum of distances, rows within the radius, their sum of d2, unsettled rows, status} -> totals
__global__ void nn_totals_kernel(const double* __restrict__ slab, int rows, const NnState* __restrict__ st, double* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t[3] = {0.0, 0.0, 0.0};
  if (st->stop == 0)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < 3; ++k) t[k] += slab[r * 4 + k];
  for (int k = 0; k < 3; ++k) totals[k] = t[k];
  totals[3] = st->stop == 0 ? static_cast<double>(st->n_list) : 0.0;
  totals[4] = static_cast<double>(st->stop);
  totals[5] = totals[6] = totals[7] = 0.0;
}

// compute_registration_rmse: |G p - E p| per row -> block slabs {sum, -, bad}
__global__ __launch_bounds__(kBlock) void realign_kernel(const float* __restrict__ pts, int n, long long ld, Mat16 G, Mat16 E,
                                                         double* __restrict__ slab) {
  double sum = 0.0, bad = 0.0;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kBlock) {
    const double x = pts[i * ld], y = pts[i * ld + 1], z = pts[i * ld + 2];
    double g[3] = {x, y, z}, e[3] = {x, y, z};
    move_row(G.v, g[0], g[1], g[2]);
    move_row(E.v, e[0], e[1], e[2]);
    const double d = sqrt(sq_dist(g[0], g[1], g[2], e[0], e[1], e[2]));
    if (!isfinite(d)) bad = 1.0;  // (a non-finite point or transform)
    else sum += d;
  }
  block_sums(sum, 0.0, bad, slab);
}

__global__ void realign_totals_kernel(const double* __restrict__ slab, int rows, double* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double sum = 0.0, bad = 0.0;
  for (int r = 0; r < rows; ++r) {
    sum += slab[r * 4];
    bad += slab[r * 4 + 2];
  }
  totals[0] = sum;
  totals[1] = bad;
}

// ---- rdm_information_matrix: the 6 x 6 information matrix of the rows under the radius --------------------------------------
// Per correspondence (i, j = idx[i]) with sqrt(d2[i]) < radius (strict; the rows nn_sum_kernel counts) and p = (x, y, z) = s'_j:
// the closed form of sum g g^T over g = (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1) needs C = sum 1 (an integer),
// s = sum p, M = sum p p^T (six entries) and, for the inlier RMSE, sum d2.
constexpr int kInfoSums = 10;  // x, y, z, xx, xy, xz, yy, yz, zz, d2
constexpr int kInfoOut = 40;   // the read-back: the matrix row-major [36], C, sum of d2, rows that took the sweep, status

// Block sums in nn_sum_kernel's order (per thread in row order, lanes by butterfly, wavefronts in order) -> slab[block][kInfoSums],
// count[block]; within[i] = 1 iff row i has a correspondence (the compaction's flags).
__global__ __launch_bounds__(kBlock) void info_sum_kernel(const double* __restrict__ d2, const int* __restrict__ idx, int n,
                                                          const double* __restrict__ sm, const NnState* __restrict__ st,
                                                          double* __restrict__ slab, long long* __restrict__ count,
                                                          uint8_t* __restrict__ within) {
  if (st->stop != 0) return;
  const double r = st->radius;
  double acc[kInfoSums];
  for (int k = 0; k < kInfoSums; ++k) acc[k] = 0.0;
  int c = 0;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * kBlock) {
    const double v = d2[i];
    const bool in = sqrt(v) < r;  // (strict; false for d2 = +inf, so idx = n_s is never read)
    within[i] = in ? 1 : 0;
    if (in) {
      const long long j = idx[i];
      const double x = sm[3 * j], y = sm[3 * j + 1], z = sm[3 * j + 2];
      c += 1;
      acc[0] += x; acc[1] += y; acc[2] += z;
      acc[3] += x * x; acc[4] += x * y; acc[5] += x * z;
      acc[6] += y * y; acc[7] += y * z; acc[8] += z * z;
      acc[9] += v;
    }
  }
  __shared__ int red_c[kRowsPerBlock];
  c = wave_sum_i(c);
  if (lane_id() == 0) red_c[threadIdx.x >> 6] = c;
  const double sum = block_sum<kInfoSums, kBlock>(acc, threadIdx.x);  // (synchronises)
  if (threadIdx.x < kInfoSums) {
    slab[blockIdx.x * kInfoSums + threadIdx.x] = sum;
  } else if (threadIdx.x == kInfoSums) {
    long long v = 0;
    for (int w = 0; w < kRowsPerBlock; ++w) v += red_c[w];
    count[blockIdx.x] = v;
  }
}

// One thread: the block slabs in order -> out[kInfoOut] (all zero but the status after a bad call, or without rows).
__global__ void info_totals_kernel(const double* __restrict__ slab, const long long* __restrict__ count, int rows,
                                   const NnState* __restrict__ st, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t[kInfoSums];
  for (int k = 0; k < kInfoSums; ++k) t[k] = 0.0;
  long long c = 0;
  if (st->stop == 0)
    for (int r = 0; r < rows; ++r) {
      for (int k = 0; k < kInfoSums; ++k) t[k] += slab[r * kInfoSums + k];
      c += count[r];
    }
  const double C = static_cast<double>(c), sx = t[0], sy = t[1], sz = t[2];
  const double xx = t[3], xy = t[4], xz = t[5], yy = t[6], yz = t[7], zz = t[8];
  const double info[36] = {yy + zz, -xy,     -xz,     0.0, -sz, sy,    //
                           -xy,     xx + zz, -yz,     sz,  0.0, -sx,   //
                           -xz,     -yz,     xx + yy, -sy, sx,  0.0,   //
                           0.0,     sz,      -sy,     C,   0.0, 0.0,   //
                           -sz,     0.0,     sx,      0.0, C,   0.0,   //
                           sy,      -sx,     0.0,     0.0, 0.0, C};
  for (int k = 0; k < 36; ++k) out[k] = info[k] + 0.0;  // (+ 0.0: no negative zeros)
  out[36] = C;
  out[37] = t[9];
  out[38] = st->stop == 0 ? static_cast<double>(st->n_list) : 0.0;
  out[39] = static_cast<double>(st->stop);
}

// out[k] = (i, idx[i]) for the k-th row under the radius, k < capacity (rows ascending: the compaction is stable)
__global__ __launch_bounds__(kBlock) void info_corr_kernel(const int* __restrict__ rows, const int* __restrict__ idx,
                                                           const NnState* __restrict__ st, long long capacity,
                                                           long long* __restrict__ out) {
  if (st->stop != 0) return;
  const long long count = st->n_corr < capacity ? st->n_corr : capacity;
  for (long long k = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; k < count; k += static_cast<long long>(gridDim.x) * kBlock) {
    const int i = rows[k];
    out[2 * k] = i;
    out[2 * k + 1] = idx[i];
  }
}

using RowIter = rocprim::counting_iterator<int>;

size_t select_temp_bytes(int64_t n) {
  size_t bytes = 0;
  if (n > 0 && rocprim::select(nullptr, bytes, RowIter(0), static_cast<const uint8_t*>(nullptr), static_cast<int*>(nullptr),
                               static_cast<unsigned*>(nullptr), static_cast<size_t>(n)) != hipSuccess)
    return 0;
  return bytes;
}

struct Work {
  double *qm, *sm;
  double *slab_q, *slab_s, *slab_sum;
  CellIndex ci;
  Rec* recs;
  NnState* st;
  double* totals;
  int* idx;
  double* d2;
  uint8_t* open;
  int* list;
  void* select_tmp;
  size_t select_bytes;
};

bool carve(Arena& ar, int64_t n, int64_t m, Work& w) {
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1), mm = static_cast<size_t>(m > 0 ? m : 1);
  w.qm = ar.take<double>(3 * nn);
  w.sm = ar.take<double>(3 * mm);
  w.slab_q = ar.take<double>(kCellMaxBlocks * 8);
  w.slab_s = ar.take<double>(kCellMaxBlocks * 8);
  w.slab_sum = ar.take<double>(kCellMaxBlocks * 4);
  carve_cell_index(ar, m, w.ci);
  w.recs = ar.take<Rec>(mm);
  w.st = ar.take<NnState>(1);
  w.totals = ar.take<double>(8);
  w.idx = ar.take<int>(nn);
  w.d2 = ar.take<double>(nn);
  w.open = ar.take<uint8_t>(nn);
  w.list = ar.take<int>(nn);
  w.select_bytes = select_temp_bytes(n);
  w.select_tmp = ar.take<char>(w.select_bytes > 0 ? w.select_bytes : 1);
  return ar.ok;
}

bool sizes_ok(int64_t n, int64_t m, int64_t ld_q, int64_t ld_s) {
  return n >= 0 && n < (1ll << 31) - 64 && m >= 0 && m < (1ll << 31) - 64 && ld_q >= 3 && ld_s >= 3;
}

unsigned row_blocks(int64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" size_t rdm_nearest_workspace_bytes(int64_t n_q, int64_t n_s) {
  using namespace rdm;
  Arena ar(nullptr, 0);
  Work w;
  carve(ar, n_q > 0 ? n_q : 0, n_s > 0 ? n_s : 0, w);
  return ar.off;
}

namespace {

// move, boxes, setup, the index of the moved support cloud, phase 1, the list of unsettled rows, phase 2: idx / d2 of every row
int search(const float* q, int n, int64_t ld_q, const float* s, int m, int64_t ld_s, const double* q_transform_host,
           const double* s_transform_host, double cell, double radius, const Work& w, int* out_idx, double* out_d2, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(cell_move_kernel<float>, dim3(row_blocks(n)), dim3(kBlock), 0, st, q, n, static_cast<long long>(ld_q),
                       mat_of(q_transform_host), q_transform_host ? 1 : 0, w.qm);
  if (m > 0)
    hipLaunchKernelGGL(cell_move_kernel<float>, dim3(row_blocks(m)), dim3(kBlock), 0, st, s, m, static_cast<long long>(ld_s),
                       mat_of(s_transform_host), s_transform_host ? 1 : 0, w.sm);
  const int qb = point_blocks(n), sb = point_blocks(m);
  hipLaunchKernelGGL(nn_box_kernel, dim3(qb), dim3(kBlock), 0, st, w.qm, n, w.slab_q);
  hipLaunchKernelGGL(nn_box_kernel, dim3(sb), dim3(kBlock), 0, st, w.sm, m, w.slab_s);
  hipLaunchKernelGGL(nn_setup_kernel, dim3(1), dim3(64), 0, st, w.slab_s, sb, m, w.slab_q, qb, cell, radius, w.ci.grid, w.st);
  if (m > 0) {
    CellIndex ci = w.ci;
    const int rc = index_cells(w.sm, m, &w.st->stop, ci, w.recs, st);
    if (rc != RDM_OK) return rc;
  }
  if (n > 0) {
    hipLaunchKernelGGL(nn_shell_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(n) + kRowsPerBlock - 1) / kRowsPerBlock)),
                       dim3(kBlock), 0, st, w.qm, n, w.ci.keys, w.recs, m, w.ci.grid, w.st, out_idx, out_d2, w.open);
    if (m > 0) {
      // (after a bad call `open` holds stale flags: the list is then garbage of at most n entries, and nothing reads it)
      size_t bytes = w.select_bytes;
      RDM_HIP_CHECK(rocprim::select(w.select_tmp, bytes, RowIter(0), static_cast<const uint8_t*>(w.open), w.list, &w.st->n_list,
                                    static_cast<size_t>(n), st));
      const int64_t groups = (static_cast<int64_t>(n) + kWave - 1) / kWave;
      hipLaunchKernelGGL(nn_sweep_kernel, dim3(static_cast<unsigned>(groups > kSweepMaxBlocks ? kSweepMaxBlocks : groups)), dim3(kBlock),
                         0, st, w.qm, w.sm, m, w.list, w.st, out_idx, out_d2);
    }
  }
  return RDM_OK;
}

struct InfoWork {
  Work nn;
  double* slab;
  long long* count;
  double* out;
};

bool carve_info(Arena& ar, int64_t n, int64_t m, InfoWork& w) {
  carve(ar, n, m, w.nn);
  w.slab = ar.take<double>(kCellMaxBlocks * kInfoSums);
  w.count = ar.take<long long>(kCellMaxBlocks);
  w.out = ar.take<double>(kInfoOut);
  return ar.ok;
}

}  // namespace

extern "C" int rdm_nearest(const float* q, int64_t n_q, int64_t ld_q, const float* s, int64_t n_s, int64_t ld_s,
                           const double* q_transform_host, const double* s_transform_host, double cell, double radius, int32_t* idx,
                           double* d2, double* totals_host, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(totals_host, "rdm_nearest: null totals_host");
  RDM_REQUIRE(sizes_ok(n_q, n_s, ld_q, ld_s), "rdm_nearest: bad sizes (n_q=%lld n_s=%lld; both < 2^31 - 64, row strides >= 3)",
              (long long)n_q, (long long)n_s);
  RDM_REQUIRE((q || n_q == 0) && (s || n_s == 0), "rdm_nearest: null points");
  RDM_REQUIRE(std::isfinite(cell) && std::isfinite(radius), "rdm_nearest: cell (%g) and radius (%g) must be finite", cell, radius);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, n_q, n_s, w)) {
    set_error("rdm_nearest: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  const int n = static_cast<int>(n_q), m = static_cast<int>(n_s);
  int* out_idx = idx ? idx : w.idx;
  double* out_d2 = d2 ? d2 : w.d2;
  int rc = search(q, n, ld_q, s, m, ld_s, q_transform_host, s_transform_host, cell, radius, w, out_idx, out_d2, st);
  if (rc != RDM_OK) return rc;
  const int qb = point_blocks(n);
  if (n > 0) hipLaunchKernelGGL(nn_sum_kernel, dim3(qb), dim3(kBlock), 0, st, out_d2, n, w.st, w.slab_sum);
  hipLaunchKernelGGL(nn_totals_kernel, dim3(1), dim3(64), 0, st, w.slab_sum, n > 0 ? qb : 0, w.st, w.totals);
  rc = launch_status("rdm_nearest");
  if (rc != RDM_OK) return rc;
  double host[8];
  RDM_HIP_CHECK(hipMemcpyAsync(host, w.totals, sizeof(host), hipMemcpyDeviceToHost, st));  // the call's one read-back
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < 5; ++k) totals_host[k] = host[k];
  if (host[4] != 0.0) {
    set_error("rdm_nearest: a point is not finite (before or after moving), or a support point lies beyond 2^30 cells (or the "
              "box beyond 2^62 cells) of the cell edge");
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}

extern "C" size_t rdm_information_workspace_bytes(int64_t n_q, int64_t n_s) {
  using namespace rdm;
  Arena ar(nullptr, 0);
  InfoWork w;
  carve_info(ar, n_q > 0 ? n_q : 0, n_s > 0 ? n_s : 0, w);
  return ar.off;
}

extern "C" int rdm_information_matrix(const float* q, int64_t n_q, int64_t ld_q, const float* s, int64_t n_s, int64_t ld_s,
                                      const double* q_transform_host, const double* s_transform_host, double cell, double radius,
                                      double* out_host, int64_t* corr_out, int64_t capacity, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(out_host, "rdm_information_matrix: null out_host");
  RDM_REQUIRE(sizes_ok(n_q, n_s, ld_q, ld_s), "rdm_information_matrix: bad sizes (n_q=%lld n_s=%lld; both < 2^31 - 64, row strides >= 3)",
              (long long)n_q, (long long)n_s);
  RDM_REQUIRE((q || n_q == 0) && (s || n_s == 0), "rdm_information_matrix: null points");
  RDM_REQUIRE(std::isfinite(cell), "rdm_information_matrix: cell (%g) must be finite", cell);
  RDM_REQUIRE(radius > 0.0 && std::isfinite(radius), "rdm_information_matrix: radius must be > 0 and finite (got %g)", radius);
  RDM_REQUIRE(capacity >= 0, "rdm_information_matrix: negative capacity");
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  InfoWork w;
  if (!carve_info(ar, n_q, n_s, w)) {
    set_error("rdm_information_matrix: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  const int n = static_cast<int>(n_q), m = static_cast<int>(n_s);
  int rc = search(q, n, ld_q, s, m, ld_s, q_transform_host, s_transform_host, cell, radius, w.nn, w.nn.idx, w.nn.d2, st);
  if (rc != RDM_OK) return rc;
  const bool rows = n > 0 && m > 0;  // (without support rows d2 = +inf: no correspondence)
  const int qb = point_blocks(n);
  if (rows) {
    // (the flags of the unsettled rows and their list are read out: both buffers now serve the rows under the radius)
    hipLaunchKernelGGL(info_sum_kernel, dim3(qb), dim3(kBlock), 0, st, w.nn.d2, w.nn.idx, n, w.nn.sm, w.nn.st, w.slab, w.count,
                       w.nn.open);
    if (corr_out) {
      size_t bytes = w.nn.select_bytes;
      RDM_HIP_CHECK(rocprim::select(w.nn.select_tmp, bytes, RowIter(0), static_cast<const uint8_t*>(w.nn.open), w.nn.list,
                                    &w.nn.st->n_corr, static_cast<size_t>(n), st));
      hipLaunchKernelGGL(info_corr_kernel, dim3(qb), dim3(kBlock), 0, st, w.nn.list, w.nn.idx, w.nn.st,
                         static_cast<long long>(capacity), reinterpret_cast<long long*>(corr_out));
    }
  }
  hipLaunchKernelGGL(info_totals_kernel, dim3(1), dim3(64), 0, st, w.slab, w.count, rows ? qb : 0, w.nn.st, w.out);
  rc = launch_status("rdm_information_matrix");
  if (rc != RDM_OK) return rc;
  double host[kInfoOut];
  RDM_HIP_CHECK(hipMemcpyAsync(host, w.out, sizeof(host), hipMemcpyDeviceToHost, st));  // the call's one read-back
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  if (host[39] != 0.0) {
    set_error("rdm_information_matrix: a point is not finite (before or after moving), or a target point lies beyond 2^30 cells "
              "(or the box beyond 2^62 cells) of the cell edge");
    return RDM_ERR_ARG;
  }
  for (int k = 0; k < kInfoOut; ++k) out_host[k] = host[k];
  if (corr_out && host[36] > static_cast<double>(capacity)) {
    set_error("rdm_information_matrix: %lld correspondences, capacity %lld", (long long)host[36], (long long)capacity);
    return RDM_ERR_CAPACITY;
  }
  return RDM_OK;
}

extern "C" int rdm_realign_error(const float* pts, int64_t n, int64_t ld, const double* gt_host, const double* est_host,
                                 double* mean_host, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(gt_host && est_host && mean_host, "rdm_realign_error: null pointer");
  RDM_REQUIRE(n >= 0 && n < (1ll << 31) - 64 && ld >= 3 && (pts || n == 0), "rdm_realign_error: bad points (n=%lld; < 2^31 - 64, row stride >= 3)",
              (long long)n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, 0, 0, w)) {
    set_error("rdm_realign_error: workspace too small (%zu < %zu bytes; rdm_nearest_workspace_bytes(0, 0))", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  const int blocks = point_blocks(n);
  hipLaunchKernelGGL(realign_kernel, dim3(blocks), dim3(kBlock), 0, st, pts, static_cast<int>(n), static_cast<long long>(ld),
                     mat_of(gt_host), mat_of(est_host), w.slab_sum);
  hipLaunchKernelGGL(realign_totals_kernel, dim3(1), dim3(64), 0, st, w.slab_sum, blocks, w.totals);
  const int rc = launch_status("rdm_realign_error");
  if (rc != RDM_OK) return rc;
  double host[2];
  RDM_HIP_CHECK(hipMemcpyAsync(host, w.totals, sizeof(host), hipMemcpyDeviceToHost, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  if (host[1] != 0.0) {
    set_error("rdm_realign_error: a point or a transform is not finite");
    return RDM_ERR_ARG;
  }
  *mean_host = host[0] / static_cast<double>(n);  // (NaN without points, as numpy's mean of nothing)
  return RDM_OK;
}
