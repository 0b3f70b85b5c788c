// Point-to-point ICP on the GPU: the refinement of the KITTI ground-truth poses
// (preporcess/generate_kitti_pairs.py:157-172: Open3D registration_icp, TransformationEstimationPointToPoint without
// scaling, ICPConvergenceCriteria, 0.5 m, up to 5000 iterations, on the raw ~120 k-point scans).
//
// Open3D (0.11) is not under the reference tree -> PARITY UNPINNED.  Restated algorithm (RegistrationICP):
//   pcd = init . source (float64; left as is for the identity), transformation = init, evaluate;
//   for i < max_iteration: update = Kabsch(correspondences) (identity if there are none), transformation = update .
//   transformation, pcd = update . pcd (incremental), evaluate; stop when |d fitness| < relative_fitness and
//   |d rmse| < relative_rmse.
//   Evaluate: for every pcd point the nearest target point with d2 < r2 -> fitness = n_corr / n_source,
//   inlier_rmse = sqrt(err2 / n_corr) (both 0 without correspondences).
// Neighbour step, defined to the bit in cell_index.h (tests/icp_restatement.py gives the same idx and d2): accept iff
//   d2 < r2 with r2 = (double)(float)(r*r) (Open3D's KDTreeFlann hands FLANN a float squared radius).
//
// Structure:
//   target index, once per call (cell_index.h): cell edge h = sqrt(r2) (1 + 1e-6) >= the search radius; the records are the
//   raw fp32 targets as float4 {x, y, z, bits of j} in key order.  A query looks its 3 x 3 cell columns up by exact key
//   (binary search of the lowest key of a column, then a forward scan).
//   per iteration, with no host synchronisation: search (applies the pending update to its pcd point first; float64
//   partials of count, err2 and the two sums to block slabs) -> one-block means -> demeaned covariance (second pass:
//   60-80 m coordinates make the one-pass formula lose digits) -> one-block finalize (Kabsch, composition,
//   convergence test, history record, outputs, `done`).  Every kernel of an iteration returns at once when `done` is
//   set; the host enqueues iterations in chunks and reads `done` once per chunk.
// Determinism: every reduction runs in a fixed order (lanes by butterfly, waves and slabs in index order); there are
// no float atomics, so two runs give the same bits.
#include "../../include/rdmnet_hip.h"
#include "common.h"
#include "procrustes.h"

#pragma clang fp contract(off)

#include "cell_index.h"

namespace {
using namespace rdm;

constexpr int kBlock = kCellBlock;
constexpr int kMaxBlocks = kCellMaxBlocks;    // slab rows: the point kernels stride over at most this many blocks
constexpr int kChunk = 32;                    // iterations enqueued between two reads of `done`
constexpr int kRecord = 15;                   // history record: fitness, rmse, n_corr, update[12]

struct IcpState {
  double T[16];   // transformation so far (row-major 4x4)
  double U[12];   // update of the last finalize (R | t, rows), applied by the next search
  double fitness, rmse;
  double err2, ms[3], mt[3];
  long long n_corr;
  int done;       // 0 running, 1 finished, 2 bad target (non-finite point or extent beyond the cell limits)
  int updates;
};

// Row-wise sum over `rows` slab rows of K doubles (one block): thread t takes rows t, t + 256, ... in order.
template <int K>
__device__ __forceinline__ double slab_sum(const double* __restrict__ slab, int rows, int k) {
  double v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = 0.0;
  for (int r = threadIdx.x; r < rows; r += kBlock)
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] += slab[static_cast<long long>(r) * K + j];
  return block_sum<K, kBlock>(v, k);
}

// ---- target index --------------------------------------------------------------------------------------------------

// One block: the cell box from the bbox slabs, and the state of a new call (T = init, nothing done).
__global__ __launch_bounds__(kBlock) void icp_setup_kernel(const double* __restrict__ slab, int rows, int m, double h, Mat16 init,
                                                           Grid* __restrict__ grid, IcpState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  const bool bad = cell_box_from_slabs(slab, rows, m, h, grid);
  for (int k = 0; k < 16; ++k) st->T[k] = init.v[k];
  for (int k = 0; k < 12; ++k) st->U[k] = (k % 5 == 0) ? 1.0 : 0.0;
  st->fitness = st->rmse = st->err2 = 0.0;
  for (int a = 0; a < 3; ++a) st->ms[a] = st->mt[a] = 0.0;
  st->n_corr = 0;
  st->updates = 0;
  st->done = bad ? 2 : 0;
}

__global__ __launch_bounds__(kBlock) void icp_records_kernel(const float* __restrict__ target, int m, long long ld,
                                                             const int* __restrict__ order, float4* __restrict__ recs) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= m) return;
  const int j = order[p];
  recs[p] = make_float4(target[j * ld], target[j * ld + 1], target[j * ld + 2], __int_as_float(j));
}

// ---- neighbour step --------------------------------------------------------------------------------------------------

// Nearest target with d2 < r2 (lowest index among equal d2), or -1; *best = its d2, *rec = its record.
__device__ int nearest(double qx, double qy, double qz, const unsigned long long* __restrict__ keys,
                       const float4* __restrict__ recs, int m, const Grid& g, double r2, double* best, float4* rec) {
  int bj = -1;
  double bd = INFINITY;
  float4 br = make_float4(0.f, 0.f, 0.f, 0.f);
  *best = bd;
  *rec = br;
  if (m == 0 || g.dims[0] == 0 || !(isfinite(qx) && isfinite(qy) && isfinite(qz))) return -1;
  const double q[3] = {qx, qy, qz};
  long long c[3];
  if (!query_cell(q, g, 1, c)) return -1;
  long long z0, z1;
  if (!ring_heights(g, c[2], 1, &z0, &z1)) return -1;
  for (long long x = c[0] - 1; x <= c[0] + 1; ++x) {
    if (x < 0 || x >= g.dims[0]) continue;
    for (long long y = c[1] - 1; y <= c[1] + 1; ++y) {
      if (y < 0 || y >= g.dims[1]) continue;
      unsigned long long klo, khi;
      column_keys(g, x, y, z0, z1, &klo, &khi);
      for (int p = lower_bound(keys, m, klo); p < m && keys[p] <= khi; ++p) {
        const float4 r = recs[p];
        const double d2 = sq_dist(qx, qy, qz, static_cast<double>(r.x), static_cast<double>(r.y), static_cast<double>(r.z));
        const int j = __float_as_int(r.w);
        if (d2 < r2 && (d2 < bd || (d2 == bd && j < bj))) {
          bd = d2;
          bj = j;
          br = r;
        }
      }
    }
  }
  *best = bd;
  *rec = br;
  return bj;
}

// One evaluation: (apply the pending update to the pcd point,) search, block partials
// {count, err2, sum pcd xyz, sum target xyz} -> slab[block][8].  d2_out: optional (-1 where there is no neighbour).
__global__ __launch_bounds__(kBlock) void icp_search_kernel(double* __restrict__ pcd, int n, int apply,
                                                            const unsigned long long* __restrict__ keys,
                                                            const float4* __restrict__ recs, int m, const Grid* __restrict__ grid,
                                                            double r2, const IcpState* __restrict__ st, int* __restrict__ idx,
                                                            double* __restrict__ d2_out, double* __restrict__ slab) {
  if (st->done) return;
  const Grid g = *grid;
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    double x = pcd[3ll * i], y = pcd[3ll * i + 1], z = pcd[3ll * i + 2];
    if (apply) {
      move_row(st->U, x, y, z);
      pcd[3ll * i] = x;
      pcd[3ll * i + 1] = y;
      pcd[3ll * i + 2] = z;
    }
    double d2;
    float4 r;
    const int j = nearest(x, y, z, keys, recs, m, g, r2, &d2, &r);
    idx[i] = j;
    if (d2_out) d2_out[i] = j >= 0 ? d2 : -1.0;
    if (j >= 0) {
      acc[0] += 1.0;
      acc[1] += d2;
      acc[2] += x;
      acc[3] += y;
      acc[4] += z;
      acc[5] += static_cast<double>(r.x);
      acc[6] += static_cast<double>(r.y);
      acc[7] += static_cast<double>(r.z);
    }
  }
  const double s = block_sum<8, kBlock>(acc, threadIdx.x);
  if (threadIdx.x < 8) slab[blockIdx.x * 8 + threadIdx.x] = s;
}

// One block: means of the correspondences from the search slabs.
__global__ __launch_bounds__(kBlock) void icp_mean_kernel(const double* __restrict__ slab, int rows, IcpState* __restrict__ st) {
  if (st->done) return;
  const double s = slab_sum<8>(slab, rows, threadIdx.x);
  __shared__ double tot[8];
  if (threadIdx.x < 8) tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = tot[0];
    st->n_corr = static_cast<long long>(cnt);
    st->err2 = tot[1];
    for (int a = 0; a < 3; ++a) {
      st->ms[a] = cnt > 0.0 ? tot[2 + a] / cnt : 0.0;
      st->mt[a] = cnt > 0.0 ? tot[5 + a] / cnt : 0.0;
    }
  }
}

// Demeaned covariance H[a][b] = sum (p - ms)_a (t - mt)_b over the correspondences -> slab[block][9].
__global__ __launch_bounds__(kBlock) void icp_cov_kernel(const double* __restrict__ pcd, int n, const float* __restrict__ target,
                                                         long long ld, const int* __restrict__ idx,
                                                         const IcpState* __restrict__ st, double* __restrict__ slab) {
  if (st->done) return;
  const double ms[3] = {st->ms[0], st->ms[1], st->ms[2]}, mt[3] = {st->mt[0], st->mt[1], st->mt[2]};
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const int j = idx[i];
    if (j < 0) continue;
    double p[3], t[3];
    for (int a = 0; a < 3; ++a) {
      p[a] = pcd[3ll * i + a] - ms[a];
      t[a] = static_cast<double>(target[j * ld + a]) - mt[a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[3 * a + b] += p[a] * t[b];
  }
  const double s = block_sum<9, kBlock>(acc, threadIdx.x);
  if (threadIdx.x < 9) slab[blockIdx.x * 9 + threadIdx.x] = s;
}

// One block, evaluation k: fitness / rmse, convergence test, Kabsch update, composition, history record k, outputs.
__global__ __launch_bounds__(kBlock) void icp_finalize_kernel(const double* __restrict__ slab, int rows, IcpState* __restrict__ st,
                                                              int k, int max_iteration, int n_source, double relative_fitness,
                                                              double relative_rmse, double* __restrict__ history,
                                                              double* __restrict__ transform, double* __restrict__ fit_rmse,
                                                              int32_t* __restrict__ stats) {
  if (st->done) return;
  const double s = slab_sum<9>(slab, rows, threadIdx.x);
  __shared__ double H[9];
  if (threadIdx.x < 9) H[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long nc = st->n_corr;
  const double fitness = nc > 0 ? static_cast<double>(nc) / static_cast<double>(n_source) : 0.0;
  const double rmse = nc > 0 ? sqrt(st->err2 / static_cast<double>(nc)) : 0.0;
  const bool converged = k > 0 && fabs(st->fitness - fitness) < relative_fitness && fabs(st->rmse - rmse) < relative_rmse;
  const bool stop = converged || k >= max_iteration || n_source == 0;
  st->fitness = fitness;
  st->rmse = rmse;
  double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (!stop) {
    if (nc > 0) {
      double h[9], R[9];
      for (int q = 0; q < 9; ++q) h[q] = H[q];
      kabsch_rotation(h, R);
      for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) U[4 * a + b] = R[3 * a + b];
        U[4 * a + 3] = st->mt[a] - ((R[3 * a] * st->ms[0] + R[3 * a + 1] * st->ms[1]) + R[3 * a + 2] * st->ms[2]);
      }
    }
    double T[16];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 4; ++b)
        T[4 * a + b] = ((U[4 * a] * st->T[b] + U[4 * a + 1] * st->T[4 + b]) + U[4 * a + 2] * st->T[8 + b]) + U[4 * a + 3] * st->T[12 + b];
    for (int b = 0; b < 4; ++b) T[12 + b] = st->T[12 + b];
    for (int q = 0; q < 16; ++q) st->T[q] = T[q];
    st->updates = k + 1;
  }
  for (int q = 0; q < 12; ++q) st->U[q] = U[q];
  if (history) {
    double* rec = history + static_cast<long long>(k) * kRecord;
    rec[0] = fitness;
    rec[1] = rmse;
    rec[2] = static_cast<double>(nc);
    for (int q = 0; q < 12; ++q) rec[3 + q] = U[q];
  }
  for (int q = 0; q < 16; ++q) transform[q] = st->T[q];
  fit_rmse[0] = fitness;
  fit_rmse[1] = rmse;
  stats[0] = st->updates;
  stats[1] = static_cast<int32_t>(nc);
  if (stop) st->done = 1;
}

// ---- host ---------------------------------------------------------------------------------------------------------------

struct Work {
  double* pcd;
  int* idx;
  double* slab;
  double* slab_cov;
  IcpState* st;
  CellIndex ci;
  float4* recs;
};

bool carve(Arena& ar, int64_t n, int64_t m, Work& w) {
  w.pcd = ar.take<double>(static_cast<size_t>(n > 0 ? n : 1) * 3);
  w.idx = ar.take<int>(n > 0 ? n : 1);
  w.slab = ar.take<double>(kMaxBlocks * 8);
  w.slab_cov = ar.take<double>(kMaxBlocks * 9);
  w.st = ar.take<IcpState>(1);
  carve_cell_index(ar, m, w.ci);
  w.recs = ar.take<float4>(static_cast<size_t>(m > 0 ? m : 1));
  return ar.ok;
}

double search_r2(double r) { return static_cast<double>(static_cast<float>(r * r)); }

// Target index and a fresh state (T = init).
int build_index(const float* target, int64_t m, int64_t ld, double r2, const Mat16& init, Work& w, hipStream_t st) {
  const double h = sqrt(r2) * (1.0 + 1e-6);
  const int tb = point_blocks(m);
  hipLaunchKernelGGL(cell_bbox_kernel<float>, dim3(tb), dim3(kBlock), 0, st, target, static_cast<int>(m),
                     static_cast<long long>(ld), h, w.slab);
  hipLaunchKernelGGL(icp_setup_kernel, dim3(1), dim3(kBlock), 0, st, w.slab, tb, static_cast<int>(m), h, init, w.ci.grid, w.st);
  if (m > 0) {
    const int rc = sort_cells(target, m, ld, &w.st->done, w.ci, st);
    if (rc != RDM_OK) return rc;
    hipLaunchKernelGGL(icp_records_kernel, dim3(static_cast<unsigned>((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, target,
                       static_cast<int>(m), static_cast<long long>(ld), w.ci.order, w.recs);
  }
  return launch_status("icp target index");
}

int read_done(const IcpState* st_dev, int* done, hipStream_t st) {
  RDM_HIP_CHECK(hipMemcpyAsync(done, &st_dev->done, sizeof(int), hipMemcpyDeviceToHost, st));
  RDM_HIP_CHECK(hipStreamSynchronize(st));
  return RDM_OK;
}

}  // namespace

extern "C" size_t rdm_icp_workspace_bytes(int64_t n_source, int64_t n_target) {
  using namespace rdm;
  Arena ar(nullptr, 0);
  Work w;
  carve(ar, n_source, n_target, w);
  return ar.off;
}

extern "C" int rdm_icp_point_to_point(const float* source, int64_t n_source, int64_t ld_source, const float* target,
                                      int64_t n_target, int64_t ld_target, double max_correspondence_distance,
                                      const double* init_host, int max_iteration, double relative_fitness, double relative_rmse,
                                      double* transform, double* fitness_rmse, int32_t* stats, double* history, void* ws,
                                      size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(transform && fitness_rmse && stats, "rdm_icp_point_to_point: null output");
  RDM_REQUIRE(max_correspondence_distance > 0.0, "rdm_icp_point_to_point: max_correspondence_distance must be > 0 (got %g)",
              max_correspondence_distance);
  RDM_REQUIRE(n_source >= 0 && n_source < (1ll << 31) && n_target >= 0 && n_target < (1ll << 31) && max_iteration >= 0 &&
                  ld_source >= 3 && ld_target >= 3 && relative_fitness >= 0.0 && relative_rmse >= 0.0,
              "rdm_icp_point_to_point: bad arguments");
  RDM_REQUIRE((source || n_source == 0) && (target || n_target == 0), "rdm_icp_point_to_point: null points");
  const Mat16 init = mat_of(init_host), eye = mat_of(nullptr);
  bool identity = true;
  for (int q = 0; q < 16; ++q) identity = identity && init.v[q] == eye.v[q];
  const double r2 = search_r2(max_correspondence_distance);
  RDM_REQUIRE(r2 > 0.0 && std::isfinite(r2), "rdm_icp_point_to_point: max_correspondence_distance^2 is not a positive float");
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, n_source, n_target, w)) {
    set_error("rdm_icp_point_to_point: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  int rc = build_index(target, n_target, ld_target, r2, init, w, st);
  if (rc != RDM_OK) return rc;
  const int n = static_cast<int>(n_source), m = static_cast<int>(n_target), pb = point_blocks(n_source);
  if (n > 0)
    hipLaunchKernelGGL(cell_move_kernel<float>, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, source, n,
                       static_cast<long long>(ld_source), init, identity ? 0 : 1, w.pcd);  // pcd = init . source (or the source as is)
  int done = 0;
  for (int k = 0; k <= max_iteration && done == 0;) {
    const int end = max_iteration - k < kChunk ? max_iteration + 1 : k + kChunk;
    for (; k < end; ++k) {
      hipLaunchKernelGGL(icp_search_kernel, dim3(pb), dim3(kBlock), 0, st, w.pcd, n, k > 0 ? 1 : 0, w.ci.keys, w.recs, m, w.ci.grid, r2,
                         w.st, w.idx, static_cast<double*>(nullptr), w.slab);
      hipLaunchKernelGGL(icp_mean_kernel, dim3(1), dim3(kBlock), 0, st, w.slab, pb, w.st);
      hipLaunchKernelGGL(icp_cov_kernel, dim3(pb), dim3(kBlock), 0, st, w.pcd, n, target, static_cast<long long>(ld_target), w.idx,
                         w.st, w.slab_cov);
      hipLaunchKernelGGL(icp_finalize_kernel, dim3(1), dim3(kBlock), 0, st, w.slab_cov, pb, w.st, k, max_iteration, n,
                         relative_fitness, relative_rmse, history, transform, fitness_rmse, stats);
    }
    rc = launch_status("rdm_icp_point_to_point");
    if (rc != RDM_OK) return rc;
    rc = read_done(w.st, &done, st);  // one 4-byte read-back per chunk
    if (rc != RDM_OK) return rc;
  }
  if (done == 2) {
    set_error("rdm_icp_point_to_point: a target point is not finite or lies beyond 2^30 cells of %g m from the origin",
              sqrt(r2));
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}

extern "C" int rdm_icp_correspondences(const double* pcd, int64_t n, const float* target, int64_t n_target, int64_t ld_target,
                                       double max_correspondence_distance, int32_t* idx, double* d2, void* ws, size_t ws_bytes,
                                       void* stream) {
  using namespace rdm;
  RDM_REQUIRE(idx && d2, "rdm_icp_correspondences: null output");
  RDM_REQUIRE(max_correspondence_distance > 0.0, "rdm_icp_correspondences: max_correspondence_distance must be > 0 (got %g)",
              max_correspondence_distance);
  RDM_REQUIRE(n >= 0 && n < (1ll << 31) && n_target >= 0 && n_target < (1ll << 31) && ld_target >= 3,
              "rdm_icp_correspondences: bad arguments");
  RDM_REQUIRE((pcd || n == 0) && (target || n_target == 0), "rdm_icp_correspondences: null points");
  const double r2 = search_r2(max_correspondence_distance);
  RDM_REQUIRE(r2 > 0.0 && std::isfinite(r2), "rdm_icp_correspondences: max_correspondence_distance^2 is not a positive float");
  hipStream_t st = static_cast<hipStream_t>(stream);
  Arena ar(ws, ws_bytes);
  Work w;
  if (!carve(ar, 0, n_target, w)) {
    set_error("rdm_icp_correspondences: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  int rc = build_index(target, n_target, ld_target, r2, mat_of(nullptr), w, st);
  if (rc != RDM_OK) return rc;
  if (n > 0)
    hipLaunchKernelGGL(icp_search_kernel, dim3(point_blocks(n)), dim3(kBlock), 0, st, const_cast<double*>(pcd), static_cast<int>(n),
                       0, w.ci.keys, w.recs, static_cast<int>(n_target), w.ci.grid, r2, w.st, idx, d2, w.slab);
  rc = launch_status("rdm_icp_correspondences");
  if (rc != RDM_OK) return rc;
  int done = 0;
  rc = read_done(w.st, &done, st);
  if (rc != RDM_OK) return rc;
  if (done == 2) {
    set_error("rdm_icp_correspondences: a target point is not finite or lies beyond 2^30 cells of %g m from the origin", sqrt(r2));
    return RDM_ERR_ARG;
  }
  return RDM_OK;
}
