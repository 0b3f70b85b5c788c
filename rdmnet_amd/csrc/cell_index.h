// Exact cell index over a point cloud and the searches on it, shared by the ICP neighbour step (icp.hip), the ball query
// (ball_query.hip) and the exact nearest neighbour (nearest.hip).
//
// Definition, to the bit (tests/icp_restatement.py, pair_overlap_restatement.py and nearest_restatement.py restate it in float64):
//   points are fp32 read as double; a transform is a row-major float64 4x4 and moves a row as
//   x' = ((R00*x + R01*y) + R02*z) + t0 (move_row);  d = query - indexed point per axis;  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
//   (sq_dist); neither is ever contracted, whatever the including file's setting.  A tie is two indexed rows with equal d2 for
//   one query: where one row is asked for, the LOWEST row wins.
//   Radius rule per client: icp.hip accepts d2 < r2 with r2 = (double)(float)(r*r) (open ball, float-rounded); ball_query.hip
//   accepts d2 <= r2 with r2 = r*r in double (closed ball); nearest.hip has no radius: the smallest d2 over all rows.
//
// Index: cell = floor(p / h) per axis -> cell box (block slabs, finalized by one thread of the client's setup kernel) -> 64-bit
//   key relative to the box, (x * dims[1] + y) * dims[2] + z -> radix sort of (key, index) -> records in key order.
// Query: its cell relative to the box (query_cell; the radius searches let it lie one cell outside, slack = 1, the exact search
//   wants it inside, slack = 0), the heights of the cube of cells within rho of it clamped to the box (ring_heights), then per
//   cell column (x, y) of that cube inside the box the key range (column_keys), looked up by exact key (lower_bound): no
//   clamping in x and y, so a query outside the box finds exactly the points within h of it, and every occupied cell holds its own points only, whatever the extent (the box only has
//   to fit 2^62 cells).  How a range is walked is the client's: one bisect and a forward scan (icp.hip), two bisects per lane and
//   a wave-wide walk (the others).
// The indexed points are rows of T (float or double) with row stride ld, read as double.  Everything here has internal linkage
// and every kernel is a template: an including file gets the kernels it launches and no others.
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

struct Mat16 {
  double v[16];  // row-major 4x4
};

inline Mat16 mat_of(const double* host) {  // (null: the identity)
  Mat16 T = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  if (host)
    for (int k = 0; k < 16; ++k) T.v[k] = host[k];
  return T;
}

struct Rec {  // an indexed (moved) point and its row, in key order
  double x, y, z;
  long long j;
};

// (x, y, z) <- M . (x, y, z, 1) for the rows R | t of M
__device__ __forceinline__ void move_row(const double* M, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  const double a = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  const double b = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  const double c = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  x = a; y = b; z = c;
}

__device__ __forceinline__ double sq_dist(double qx, double qy, double qz, double sx, double sy, double sz) {
#pragma clang fp contract(off)
  const double dx = qx - sx, dy = qy - sy, dz = qz - sz;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// moved[j] = M . pts[j] (or pts[j] as it is), float64 [n, 3]
template <typename T>
__global__ __launch_bounds__(kCellBlock) void cell_move_kernel(const T* __restrict__ pts, int n, long long ld, Mat16 M, int apply,
                                                               double* __restrict__ moved) {
  const long long j = static_cast<long long>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (j >= n) return;
  double x = pts[j * ld], y = pts[j * ld + 1], z = pts[j * ld + 2];
  if (apply) move_row(M.v, x, y, z);
  moved[3 * j] = x;
  moved[3 * j + 1] = y;
  moved[3 * j + 2] = z;
}

// The block's box: lowest lo, highest hi and highest bad over its threads (serial over t = 0..255 per value) -> slab[block][8].
__device__ __forceinline__ void block_box(const double (&lo)[3], const double (&hi)[3], double bad, double* __restrict__ slab) {
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
  block_box(lo, hi, bad, slab);
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

// records in key order: recs[p] = {moved[order[p]], order[p]}; nothing when *stop != 0
template <typename T>
__global__ __launch_bounds__(kCellBlock) void cell_records_kernel(const T* __restrict__ moved, int m, const int* __restrict__ order,
                                                                  const int* __restrict__ stop, Rec* __restrict__ recs) {
  const long long p = static_cast<long long>(blockIdx.x) * kCellBlock + threadIdx.x;
  if (p >= m || *stop != 0) return;
  const long long j = order[p];
  recs[p] = Rec{moved[3 * j], moved[3 * j + 1], moved[3 * j + 2], j};
}

// The query's cell relative to the box -> c; false when no occupied cell lies within `slack` (0 or 1) cells of it.
__device__ __forceinline__ bool query_cell(const double (&q)[3], const Grid& g, int slack, long long (&c)[3]) {
  bool near = true;
  for (int a = 0; a < 3; ++a) {
    const double ca = cell_of(q[a], g.h) - static_cast<double>(g.lo[a]);  // (exact while the query is within 2^52 cells; beyond: false)
    const double d = static_cast<double>(g.dims[a]);
    if (slack ? (ca >= -1.0 && ca <= d) : (ca >= 0.0 && ca < d)) c[a] = static_cast<long long>(ca);
    else near = false;
  }
  return near;
}

// The heights of the cube of cells within rho of a cell at height cz, clamped to the box: [*z0, *z1]; false when there is none.
__device__ __forceinline__ bool ring_heights(const Grid& g, long long cz, int rho, long long* z0, long long* z1) {
  *z0 = cz - rho < 0 ? 0 : cz - rho;
  *z1 = cz + rho >= g.dims[2] ? g.dims[2] - 1 : cz + rho;
  return *z0 <= *z1;
}

// Cell column (x, y) of the box (0 <= x < dims[0], 0 <= y < dims[1]: the caller's test, columns are not clamped) over the heights
// [z0, z1]: its keys [*klo, *khi].  Ascending keys are x-major columns, then z.
__device__ __forceinline__ void column_keys(const Grid& g, long long x, long long y, long long z0, long long z1, unsigned long long* klo,
                                            unsigned long long* khi) {
  const long long col = (x * g.dims[1] + y) * g.dims[2];
  *klo = static_cast<unsigned long long>(col + z0);
  *khi = static_cast<unsigned long long>(col + z1);
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

// The whole index of a float64 [m, 3] cloud: keys, their sort and the records in key order.
template <typename T>
inline int index_cells(const T* moved, int64_t m, const int* stop, CellIndex& c, Rec* recs, hipStream_t st) {
  if (m <= 0) return RDM_OK;
  const int rc = sort_cells(moved, m, 3, stop, c, st);
  if (rc != RDM_OK) return rc;
  hipLaunchKernelGGL(cell_records_kernel<T>, dim3(static_cast<unsigned>((m + kCellBlock - 1) / kCellBlock)), dim3(kCellBlock), 0, st, moved,
                     static_cast<int>(m), c.order, stop, recs);
  return RDM_OK;
}

}  // namespace
}  // namespace rdm
