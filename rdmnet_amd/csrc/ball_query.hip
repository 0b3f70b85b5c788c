// Ground-truth point correspondences and cloud overlap: get_correspondences and compute_overlap
// (geotransformer/utils/registration.py:191-216, a cKDTree ball query / nearest neighbour between two full clouds) as one
// fixed-radius ball query on the GPU.
//
// Definition, to the bit (x', d2 and ties: cell_index.h; tests/pair_overlap_restatement.py is the float64 numpy restatement):
//   the transform moves src (null: src as it is);  d = ref - src' per axis;  r2 = r*r in double (NOT icp.hip's float-rounded r2);
//   (i, j) is a correspondence iff d2 <= r2 (cKDTree's ball is closed); the list is int64 [C, 2] in ascending (i, j) -- cKDTree
//   leaves the order inside a row open, this library defines it as ascending j;
//   a row overlaps iff the smallest d2 of its correspondences satisfies sqrt(d2) < r (compute_overlap's comparison is strict;
//   a row without a correspondence has no point of the other cloud within r, so it does not overlap).
//
// Structure:
//   index of the MOVED src cloud, once per call (cell_index.h): cell edge h = r (1 + 1e-6) >= r.  A ref row finds its
//   candidates in the 3 x 3 cell columns around its own cell, by exact key.
//   pass 1 (ball_count_kernel), one wavefront per ref row: lanes 0..8 bisect one column each, then the wave walks the nine
//   candidate ranges 64 records at a time -> count, smallest d2 (-1 if none), and per src row found a hit byte (d2 <= r2) and a
//   near byte (sqrt(d2) < r), plain stores of 1 (all writers write the same value).
//   scan: device-wide exclusive scan of the counts into int64 offsets (offsets[n] = C); ball_totals_kernel counts the
//   overlapping rows of both sides (integer atomics, one per wave) and gathers {C, ref rows, src rows, status}.
//   pass 2 (ball_fill_kernel), one wavefront per ref row, any row length: the same walk writes the row's src indices in arrival
//   (cell-key) order into column 0 of the row's own output segment by ballot prefix; then entry k goes to position
//   #{k' : j_k' < j_k} of column 1 (the indices of a row are distinct, so the ranks are a permutation), and column 0 is
//   overwritten with i.  No cap on the length of a row, no scratch beyond the output itself.
// Determinism: counts, minima (fmin is exact) and ranks do not depend on scheduling; the only atomics are integer adds.
// A src point that is not finite or beyond the cell limits (or a moved one: a non-finite transform), and a ref point that is
// not finite, give status 2: the count call returns RDM_ERR_ARG, no kernel indexes anything by such a point.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/rdmnet_hip.h"
#include "common.h"

#pragma clang fp contract(off)

#include "cell_index.h"

namespace {
using namespace rdm;

constexpr int kBlock = kCellBlock;
constexpr int kRowsPerBlock = kBlock / kWave;  // ref rows (wavefronts) per workgroup

struct BallState {
  double r, r2;
  int stop;     // 2: a bad src cloud (cell_index.h), set by the setup kernel before anything reads the index
  int bad_ref;  // 2: a non-finite ref point (plain store by pass 1)
};

struct ToLong {
  __host__ __device__ long long operator()(int v) const { return static_cast<long long>(v); }
};
using CountIter = rocprim::transform_iterator<const int*, ToLong, long long>;

// One thread: the cell box of the moved cloud, the state of a new call, zeroed totals.
__global__ void ball_setup_kernel(const double* __restrict__ slab, int rows, int m, double h, double r, Grid* __restrict__ grid,
                                  BallState* __restrict__ st, long long* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool bad = cell_box_from_slabs(slab, rows, m, h, grid);
  st->r = r;
  st->r2 = r * r;
  st->stop = bad ? 2 : 0;
  st->bad_ref = 0;
  for (int k = 0; k < 4; ++k) totals[k] = 0;
}

// The candidate ranges of one ref row, wave-wide: lane c < 9 holds [begin, end) of cell column c (x-major, so ascending keys);
// every other lane, and a column outside the box, an empty range.  Returns false when the row is not finite.
__device__ __forceinline__ bool column_ranges(double qx, double qy, double qz, const unsigned long long* __restrict__ keys, int m,
                                              const Grid& g, int lane, int* begin, int* end) {
  *begin = *end = 0;
  if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) return false;
  if (m == 0 || g.dims[0] == 0 || lane >= 9) return true;
  const double q[3] = {qx, qy, qz};
  long long c[3], z0, z1;
  if (!query_cell(q, g, 1, c)) return true;  // no occupied cell next to the row's
  const bool some = ring_heights(g, c[2], 1, &z0, &z1);
  const long long x = c[0] - 1 + lane / 3, y = c[1] - 1 + lane % 3;
  if (!some || x < 0 || x >= g.dims[0] || y < 0 || y >= g.dims[1]) return true;
  unsigned long long klo, khi;
  column_keys(g, x, y, z0, z1, &klo, &khi);
  *begin = lower_bound(keys, m, klo);
  *end = lower_bound(keys, m, khi + 1);
  return true;
}

// Pass 1: one wavefront per ref row.
__global__ __launch_bounds__(kBlock) void ball_count_kernel(const float* __restrict__ ref, int n, long long ld,
                                                            const unsigned long long* __restrict__ keys,
                                                            const Rec* __restrict__ recs, int m, const Grid* __restrict__ grid,
                                                            BallState* __restrict__ st, int* __restrict__ counts,
                                                            double* __restrict__ min_d2, uint8_t* __restrict__ ref_hit,
                                                            uint8_t* __restrict__ src_hit, uint8_t* __restrict__ src_near) {
  const int lane = lane_id();
  const long long i = static_cast<long long>(blockIdx.x) * kRowsPerBlock + (threadIdx.x >> 6);
  if (i >= n) return;  // (wave-uniform)
  int count = 0;
  double best = INFINITY;
  if (st->stop == 0) {
    const Grid g = *grid;
    const double r = st->r, r2 = st->r2;
    const double qx = ref[i * ld], qy = ref[i * ld + 1], qz = ref[i * ld + 2];
    int begin, end;
    if (!column_ranges(qx, qy, qz, keys, m, g, lane, &begin, &end) && lane == 0) st->bad_ref = 2;
    for (int c = 0; c < 9; ++c) {
      const int b = __shfl(begin, c, 64), e = __shfl(end, c, 64);
      for (int p0 = b; p0 < e; p0 += kWave) {  // (wave-uniform bounds)
        const int p = p0 + lane;
        bool hit = false;
        if (p < e) {
          const Rec s = recs[p];
          const double d2 = sq_dist(qx, qy, qz, s.x, s.y, s.z);
          hit = d2 <= r2;
          if (hit) {
            best = fmin(best, d2);
            src_hit[s.j] = 1;
            if (sqrt(d2) < r) src_near[s.j] = 1;
          }
        }
        count += __popcll(__ballot(hit));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmin(best, __shfl_xor(best, o, 64));
  }
  if (lane == 0) {
    counts[i] = count;
    min_d2[i] = count > 0 ? best : -1.0;
    if (ref_hit) ref_hit[i] = count > 0 ? 1 : 0;
  }
}

// {C, overlapping ref rows, overlapping src rows, status} -> totals (zeroed by the setup kernel)
__global__ __launch_bounds__(kBlock) void ball_totals_kernel(const double* __restrict__ min_d2, int n, const uint8_t* __restrict__ src_near,
                                                             int m, const long long* __restrict__ offsets,
                                                             const BallState* __restrict__ st, long long* __restrict__ totals) {
  const double r = st->r;
  const long long total = static_cast<long long>(n) + m;
  for (long long t0 = static_cast<long long>(blockIdx.x) * kBlock; t0 < total; t0 += static_cast<long long>(gridDim.x) * kBlock) {
    const long long t = t0 + threadIdx.x;
    bool ref_near = false, s_near = false;
    if (t < n) {
      const double d2 = min_d2[t];
      ref_near = d2 >= 0.0 && sqrt(d2) < r;
    } else if (t < total) {
      s_near = src_near[t - n] != 0;
    }
    const unsigned long long br = __ballot(ref_near), bs = __ballot(s_near);
    if (lane_id() == 0) {
      if (br) atomicAdd(reinterpret_cast<unsigned long long*>(totals + 1), static_cast<unsigned long long>(__popcll(br)));
      if (bs) atomicAdd(reinterpret_cast<unsigned long long*>(totals + 2), static_cast<unsigned long long>(__popcll(bs)));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = offsets[n];
    totals[3] = st->stop != 0 ? st->stop : st->bad_ref;
  }
}

// Pass 2: one wavefront per workgroup and ref row (the barriers below order the wave's own global stores and loads).
__global__ __launch_bounds__(kWave) void ball_fill_kernel(const float* __restrict__ ref, int n, long long ld,
                                                          const unsigned long long* __restrict__ keys, const Rec* __restrict__ recs,
                                                          int m, const Grid* __restrict__ grid, const BallState* __restrict__ st,
                                                          const int* __restrict__ counts, const long long* __restrict__ offsets,
                                                          long long* __restrict__ out, long long capacity) {
  if (st->stop != 0 || st->bad_ref != 0) return;
  const Grid g = *grid;
  const double r2 = st->r2;
  const int lane = threadIdx.x;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {  // (block-uniform)
    const int cnt = counts[i];
    const long long off = offsets[i];
    if (cnt == 0 || off + cnt > capacity) continue;
    long long* seg = out + 2 * off;  // [cnt, 2]
    const double qx = ref[i * ld], qy = ref[i * ld + 1], qz = ref[i * ld + 2];
    int begin, end;
    column_ranges(qx, qy, qz, keys, m, g, lane, &begin, &end);
    int pos = 0;
    for (int c = 0; c < 9; ++c) {
      const int b = __shfl(begin, c, 64), e = __shfl(end, c, 64);
      for (int p0 = b; p0 < e; p0 += kWave) {
        const int p = p0 + lane;
        bool hit = false;
        long long j = 0;
        if (p < e) {
          const Rec s = recs[p];
          hit = sq_dist(qx, qy, qz, s.x, s.y, s.z) <= r2;
          j = s.j;
        }
        const unsigned long long bal = __ballot(hit);
        const int k = pos + __popcll(bal & ((1ull << lane) - 1ull));
        if (hit && k < cnt) seg[2 * k] = j;  // (k < cnt always: the same walk counted the row)
        pos += __popcll(bal);
      }
    }
    __syncthreads();
    for (int k = lane; k < cnt; k += kWave) {
      const long long j = seg[2 * k];
      int rank = 0;
      for (int t = 0; t < cnt; ++t) rank += seg[2 * t] < j ? 1 : 0;
      seg[2 * rank + 1] = j;
    }
    __syncthreads();
    for (int k = lane; k < cnt; k += kWave) seg[2 * k] = i;
  }
}

struct Work {
  double* moved;
  double* slab;
  CellIndex ci;
  Rec* recs;
  BallState* st;
  long long* totals;
  int* counts;           // [n + 1], counts[n] = 0
  long long* offsets;    // [n + 1], offsets[n] = C
  double* min_d2;
  uint8_t *src_hit, *src_near;
  void* scan_tmp;
  size_t scan_bytes;
};

size_t scan_temp_bytes(int64_t n) {
  size_t bytes = 0;
  if (rocprim::exclusive_scan(nullptr, bytes, CountIter(nullptr, ToLong()), static_cast<long long*>(nullptr), 0ll,
                              static_cast<size_t>(n + 1), rocprim::plus<long long>()) != hipSuccess)
    return 0;
  return bytes;
}

bool carve(Arena& ar, int64_t n, int64_t m, Work& w) {
  const size_t mm = static_cast<size_t>(m > 0 ? m : 1), nn = static_cast<size_t>(n) + 1;
  w.moved = ar.take<double>(3 * mm);
  w.slab = ar.take<double>(kCellMaxBlocks * 8);
  carve_cell_index(ar, m, w.ci);
  w.recs = ar.take<Rec>(mm);
  w.st = ar.take<BallState>(1);
  w.totals = ar.take<long long>(4);
  w.counts = ar.take<int>(nn);
  w.offsets = ar.take<long long>(nn);
  w.min_d2 = ar.take<double>(nn);
  w.src_hit = ar.take<uint8_t>(align_up(mm, 4));
  w.src_near = ar.take<uint8_t>(align_up(mm, 4));
  w.scan_bytes = scan_temp_bytes(n);
  w.scan_tmp = ar.take<char>(w.scan_bytes > 0 ? w.scan_bytes : 1);
  return ar.ok;
}

bool sizes_ok(int64_t n, int64_t m, int64_t ld_ref, int64_t ld_src) {
  return n >= 0 && n < (1ll << 31) - 64 && m >= 0 && m < (1ll << 31) - 64 && ld_ref >= 3 && ld_src >= 3;
}

}  // namespace

extern "C" size_t rdm_ball_workspace_bytes(int64_t n_ref, int64_t n_src) {
  using namespace rdm;
  Arena ar(nullptr, 0);
  Work w;
  carve(ar, n_ref > 0 ? n_ref : 0, n_src, w);
  return ar.off;
}

extern "C" int rdm_ball_count(const float* ref, int64_t n_ref, int64_t ld_ref, const float* src, int64_t n_src, int64_t ld_src,
                              const double* transform_host, double radius, double* ref_min_d2, uint8_t* ref_hit, uint8_t* src_hit,
                              int64_t* totals_host, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(totals_host, "rdm_ball_count: null totals_host");
  RDM_REQUIRE(radius > 0.0 && std::isfinite(radius * radius), "rdm_ball_count: radius must be > 0 and finite (got %g)", radius);
  RDM_REQUIRE(sizes_ok(n_ref, n_src, ld_ref, ld_src), "rdm_ball_count: bad sizes (n_ref=%lld n_src=%lld; both < 2^31 - 64, row strides >= 3)",
              (long long)n_ref, (long long)n_src);
  RDM_REQUIRE((ref || n_ref == 0) && (src || n_src == 0), "rdm_ball_count: null points");
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, n_ref, n_src, w)) {
    set_error("rdm_ball_count: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  const int n = static_cast<int>(n_ref), m = static_cast<int>(n_src);
  const double h = radius * (1.0 + 1e-6);
  if (!src_hit) src_hit = w.src_hit;
  if (!ref_min_d2) ref_min_d2 = w.min_d2;
  // index of the moved src cloud
  if (m > 0)
    hipLaunchKernelGGL(cell_move_kernel<float>, dim3(static_cast<unsigned>((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, src, m,
                       static_cast<long long>(ld_src), mat_of(transform_host), transform_host ? 1 : 0, w.moved);
  const int tb = point_blocks(m);
  hipLaunchKernelGGL(cell_bbox_kernel<double>, dim3(tb), dim3(kBlock), 0, st, w.moved, m, 3ll, h, w.slab);
  hipLaunchKernelGGL(ball_setup_kernel, dim3(1), dim3(64), 0, st, w.slab, tb, m, h, radius, w.ci.grid, w.st, w.totals);
  if (m > 0) {
    const int rc = index_cells(w.moved, m, &w.st->stop, w.ci, w.recs, st);
    if (rc != RDM_OK) return rc;
    fill_words(reinterpret_cast<uint32_t*>(src_hit), (static_cast<int64_t>(m) + 3) / 4, 0u, st);  // (callers' buffers hold align_up(m, 4) bytes)
    fill_words(reinterpret_cast<uint32_t*>(w.src_near), (static_cast<int64_t>(m) + 3) / 4, 0u, st);
  }
  // pass 1, offsets, totals
  if (n > 0)
    hipLaunchKernelGGL(ball_count_kernel, dim3(static_cast<unsigned>((n + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(kBlock), 0, st,
                       ref, n, static_cast<long long>(ld_ref), w.ci.keys, w.recs, m, w.ci.grid, w.st, w.counts, ref_min_d2, ref_hit,
                       src_hit, w.src_near);
  fill_words(w.counts + n, 1, 0, st);
  size_t bytes = w.scan_bytes;
  RDM_HIP_CHECK(rocprim::exclusive_scan(w.scan_tmp, bytes, CountIter(w.counts, ToLong()), w.offsets, 0ll,
                                        static_cast<size_t>(n) + 1, rocprim::plus<long long>(), st));
  const long long total = static_cast<long long>(n) + m;
  const long long blocks = (total + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(ball_totals_kernel, dim3(static_cast<unsigned>(blocks < 1 ? 1 : (blocks > kCellMaxBlocks ? kCellMaxBlocks : blocks))),
                     dim3(kBlock), 0, st, ref_min_d2, n, w.src_near, m, w.offsets, w.st, w.totals);
  int rc = launch_status("rdm_ball_count");
  if (rc != RDM_OK) return rc;
  long long host[4];
  RDM_HIP_CHECK(hipMemcpyAsync(host, w.totals, sizeof(host), hipMemcpyDeviceToHost, st));  // the call's one read-back
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < 4; ++k) totals_host[k] = host[k];
  if (host[3] != 0) {
    set_error("rdm_ball_count: a point is not finite, or a (moved) src point lies beyond 2^30 cells of %g m from the origin", radius);
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}

extern "C" int rdm_ball_fill(const float* ref, int64_t n_ref, int64_t ld_ref, int64_t n_src, int64_t* out, int64_t capacity, void* ws,
                             size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(sizes_ok(n_ref, n_src, ld_ref, 3) && capacity >= 0, "rdm_ball_fill: bad sizes");
  RDM_REQUIRE((ref || n_ref == 0) && (out || capacity == 0), "rdm_ball_fill: null pointer");
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, n_ref, n_src, w)) {
    set_error("rdm_ball_fill: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  if (n_ref == 0 || capacity == 0) return RDM_OK;
  const unsigned blocks = static_cast<unsigned>(n_ref < 65536 ? n_ref : 65536);
  hipLaunchKernelGGL(ball_fill_kernel, dim3(blocks), dim3(kWave), 0, static_cast<hipStream_t>(stream), ref, static_cast<int>(n_ref),
                     static_cast<long long>(ld_ref), w.ci.keys, w.recs, static_cast<int>(n_src), w.ci.grid, w.st, w.counts, w.offsets,
                     reinterpret_cast<long long*>(out), static_cast<long long>(capacity));
  return launch_status("rdm_ball_fill");
}
