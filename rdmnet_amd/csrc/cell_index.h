// Exact cell index over a point cloud, shared by the ICP neighbour step (icp.hip) and the ball query (ball_query.hip).
//   cell = floor(p / h) per axis -> cell box (block slabs, finalized by one thread) -> 64-bit key relative to the box ->
//   radix sort of (key, index).  A query looks its 3 x 3 cell columns up by exact key (lower_bound of the lowest key of a
//   column, then a forward scan): no clamping, so a query outside the box finds exactly the points within h of it, and every
//   occupied cell holds its own points only, whatever the extent (the box only has to fit 2^62 cells).
// The points are rows of T (float or double) with row stride ld, read as double.  Everything here has internal linkage: each
// including file gets its own kernels, and must set `#pragma clang fp contract(off)` before the include if it relies on it.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace rdm {
namespace {

constexpr int kCellBlock = 256;
constexpr int kCellMaxBlocks = 1024;             // slab rows: the point kernels stride over at most this many blocks
constexpr double kCellLimit = 1073741824.0;      // |p / h| < 2^30 for every indexed point

struct Grid {
  long long lo[3], dims[3];  // cell box of the indexed cloud (dims = 0 when it is empty or bad)
  double h;
};

__device__ __forceinline__ double cell_of(double x, double h) { return floor(x / h); }

// Per block: lowest and highest cell per axis and a bad flag (a non-finite point, or one beyond the cell limit) -> slab[block][8].
template <typename T>
__global__ __launch_bounds__(kCellBlock) void cell_bbox_kernel(const T* __restrict__ pts, int m, long long ld, double h,
                                                               double* __restrict__ slab) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.0;
  for (int j = blockIdx.x * kCellBlock + threadIdx.x; j < m; j += gridDim.x * kCellBlock) {
    for (int a = 0; a < 3; ++a) {
      const double c = cell_of(static_cast<double>(pts[j * ld + a]), h);
      if (!(fabs(c) < kCellLimit)) bad = 1.0;  // (NaN and infinities too)
      lo[a] = fmin(lo[a], c);
      hi[a] = fmax(hi[a], c);
    }
  }
  __shared__ double red[7][kCellBlock];
  for (int a = 0; a < 3; ++a) {
    red[a][threadIdx.x] = lo[a];
    red[3 + a][threadIdx.x] = hi[a];
  }
  red[6][threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    double v = red[k][0];
    for (int t = 1; t < kCellBlock; ++t) v = k < 3 ? fmin(v, red[k][t]) : fmax(v, red[k][t]);
    slab[blockIdx.x * 8 + k] = v;
  }
}

// One thread: the cell box from the bbox slabs -> *grid; returns whether the cloud is bad (non-finite, beyond the limits).
__device__ inline bool cell_box_from_slabs(const double* __restrict__ slab, int rows, int m, double h, Grid* __restrict__ grid) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool bad = false;
  for (int r = 0; r < rows; ++r) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = fmin(lo[a], slab[r * 8 + a]);
      hi[a] = fmax(hi[a], slab[r * 8 + 3 + a]);
    }
    bad = bad || slab[r * 8 + 6] != 0.0;
  }
  double cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double d = m > 0 && !bad ? hi[a] - lo[a] + 1.0 : 0.0;
    grid->lo[a] = m > 0 && !bad ? static_cast<long long>(lo[a]) : 0;
    grid->dims[a] = static_cast<long long>(d);
    cells *= d;
  }
  if (cells > 4611686018427387904.0) bad = true;  // keys are 64-bit: the box must fit 2^62 cells
  grid->h = h;
  return bad;
}

// (key, index) per point; key 0 when *stop != 0 (a bad cloud: its cells are not to be trusted)
template <typename T>
__global__ __launch_bounds__(kCellBlock) void cell_key_kernel(const T* __restrict__ pts, int m, long long ld,
                                                              const Grid* __restrict__ grid, const int* __restrict__ stop,
                                                              unsigned long long* __restrict__ keys, int* __restrict__ vals) {
  const int j = blockIdx.x * kCellBlock + threadIdx.x;
  if (j >= m) return;
  unsigned long long key = 0;
  if (*stop == 0) {
    long long c[3];
    for (int a = 0; a < 3; ++a)
      c[a] = static_cast<long long>(cell_of(static_cast<double>(pts[j * ld + a]), grid->h)) - grid->lo[a];
    key = static_cast<unsigned long long>((c[0] * grid->dims[1] + c[1]) * grid->dims[2] + c[2]);
  }
  keys[j] = key;
  vals[j] = j;
}

__device__ __forceinline__ int lower_bound(const unsigned long long* __restrict__ keys, int m, unsigned long long key) {
  int lo = 0, n = m;
  while (n > 0) {
    const int half = n >> 1;
    if (keys[lo + half] < key) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

inline int point_blocks(int64_t n) {
  const int64_t b = (n + kCellBlock - 1) / kCellBlock;
  return static_cast<int>(b < 1 ? 1 : (b > kCellMaxBlocks ? kCellMaxBlocks : b));
}

inline size_t sort_temp_bytes(int64_t m) {
  size_t bytes = 0;
  if (m > 0 &&
      rocprim::radix_sort_pairs(nullptr, bytes, static_cast<const unsigned long long*>(nullptr),
                                static_cast<unsigned long long*>(nullptr), static_cast<const int*>(nullptr),
                                static_cast<int*>(nullptr), static_cast<unsigned>(m)) != hipSuccess)
    return 0;
  return bytes;
}

// The sorted index of a cloud: keys ascending, order[p] = the point at position p.
struct CellIndex {
  Grid* grid;
  unsigned long long *keys_in, *keys;
  int *vals_in, *order;
  void* sort_tmp;
  size_t sort_bytes;
};

inline void carve_cell_index(Arena& ar, int64_t m, CellIndex& c) {
  c.grid = ar.take<Grid>(1);
  const size_t mm = static_cast<size_t>(m > 0 ? m : 1);
  c.keys_in = ar.take<unsigned long long>(mm);
  c.keys = ar.take<unsigned long long>(mm);
  c.vals_in = ar.take<int>(mm);
  c.order = ar.take<int>(mm);
  c.sort_bytes = sort_temp_bytes(m);
  c.sort_tmp = ar.take<char>(c.sort_bytes > 0 ? c.sort_bytes : 1);
}

// Keys and their sort, after the caller's setup kernel has written *c.grid and *stop from the bbox slabs.
template <typename T>
inline int sort_cells(const T* pts, int64_t m, int64_t ld, const int* stop, CellIndex& c, hipStream_t st) {
  if (m <= 0) return RDM_OK;
  const unsigned blocks = static_cast<unsigned>((m + kCellBlock - 1) / kCellBlock);
  hipLaunchKernelGGL(cell_key_kernel<T>, dim3(blocks), dim3(kCellBlock), 0, st, pts, static_cast<int>(m), static_cast<long long>(ld),
                     c.grid, stop, c.keys_in, c.vals_in);
  size_t bytes = c.sort_bytes;
  RDM_HIP_CHECK(rocprim::radix_sort_pairs(c.sort_tmp, bytes, c.keys_in, c.keys, c.vals_in, c.order, static_cast<unsigned>(m), 0u, 64u,
                                          st));
  return RDM_OK;
}

}  // namespace
}  // namespace rdm
