// Ground-truth superpoint correspondences: get_node_correspondences (geotransformer/modules/registration/matching.py:
// 252-350) as test.py's evaluation forward calls it (experiments/model.py:283-295).  An INDEX output: the arithmetic
// restates the reference's fp32 CPU arithmetic literally, operation by operation (no contraction):
//   apply_transform (modules/ops/transformation.py:7-60): q_j = fma(p2,R[j][2], fma(p1,R[j][1], p0*R[j][0])) + t_j
//     (the sgemm order for k = 3, then the separate broadcast addition);
//   patch radius: |p - node| = sqrt((dx*dx + dy*dy) + dz*dz) (torch.linalg.norm's sequential inner reduction over the
//     3 components), masked slots 0, max over the patch;
//   sphere test: ((r_ref + r_src) + (float)pos_radius) - sqrt(pairwise_distance(node_r, node_s)) > 0, AND both node masks;
//   point test: pairwise_distance(ref_pt, src_pt) < (float)(pos_radius^2) for valid slot pairs (masked pairs are 1e12 in the
//     reference, i.e. never below r^2);
//   overlap = (ref_hits / n_ref_valid + src_hits / n_src_valid) / 2 in fp32 (correctly rounded division).
// pairwise_distance is ref_sq_dist (common.h), the statement point_to_node uses.  Verified bit for bit against the
// reference on tests/golden/gt_node_corr.npz.
//
// Mapping (MI355X: 64-lane wavefronts, 160 KB LDS per CU): one wavefront per (ref node, src node) pair of the M x N grid,
// grid-stride.  The wave first runs the sphere test (wave-uniform); a pair that fails costs a handful of instructions.  A
// candidate stages its src patch (transformed, with |y|^2) in 2 KB of LDS, each lane keeps two ref points in registers
// (slots l and l + 64), and the wave walks the 128 src points: per src point two distance tests per lane, the row hits
// accumulate per lane, the column hit is one ballot -- the counts are popcounts.  The overlap (or 0 for a non-candidate)
// lands in a row-major [M, N] buffer and each ref row counts its pairs with overlap > 0; then one workgroup per ref row
// writes its entries > 0 in (ref, src) order -- torch.nonzero's order -- from the sum of the rows before it, never past
// `capacity`.  The per-node radii run one wavefront per node (two slots per lane, a max reduction).  Measured on the
// fixture's pairs (M x N = 48 k ... 116 k superpoint pairs, B ~ 10^3 candidates): tens of microseconds per pair.
#pragma clang fp contract(off)

#include "../../include/rdmnet_hip.h"
#include "common.h"

namespace {

using namespace rdm;

constexpr int kMaxK = 128;       // two patch slots per lane

struct GtArgs {
  const float* nodes[2];      // [m,3] / [n,3]
  const float* pts[2];        // idx == null: gathered patch points [m*k, 3]; else the cloud's points [n_pts, 3]
  const int64_t* idx[2];      // [m, k] indices into pts (pad index n_pts -> the zero row, as index_select on padded points)
  int64_t n_pts[2];
  const uint8_t* node_mask[2];  // null = all valid
  const uint8_t* knn_mask[2];   // null = all valid
  int cnt[2];                 // m, n
  int k;
  const float* T;             // device 4x4 row-major, src -> ref
  float radius, r2;
  float4* node4[2];           // ws: node (src transformed) + |node|^2
  float* rad[2];              // ws: max patch radius per node
  float* ov;                  // ws: [m*n] overlap, 0 for non-candidates
  int32_t* row_count;         // ws: [m] pairs with overlap > 0 per ref node
  int32_t* counts;            // device {C, B}
};

__device__ __forceinline__ float3 transform_point(const float* T, float3 p) {
  float3 q;
  q.x = fmaf(p.z, T[2], fmaf(p.y, T[1], p.x * T[0])) + T[3];
  q.y = fmaf(p.z, T[6], fmaf(p.y, T[5], p.x * T[4])) + T[7];
  q.z = fmaf(p.z, T[10], fmaf(p.y, T[9], p.x * T[8])) + T[11];
  return q;
}

// patch slot s of node u in cloud c (src transformed); the pad row is zero BEFORE the transform, as in the reference
__device__ __forceinline__ float3 slot_point(const GtArgs& a, int c, int u, int s) {
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (a.idx[c] == nullptr) {
    const float* q = a.pts[c] + 3 * (static_cast<int64_t>(u) * a.k + s);
    p = make_float3(q[0], q[1], q[2]);
  } else {
    const int64_t i = a.idx[c][static_cast<int64_t>(u) * a.k + s];
    if (i >= 0 && i < a.n_pts[c]) {
      const float* q = a.pts[c] + 3 * i;
      p = make_float3(q[0], q[1], q[2]);
    }
  }
  return c == 1 ? transform_point(a.T, p) : p;
}

__device__ __forceinline__ bool slot_valid(const GtArgs& a, int c, int u, int s) {
  return a.knn_mask[c] == nullptr || a.knn_mask[c][static_cast<int64_t>(u) * a.k + s] != 0;
}

__device__ __forceinline__ float sq_norm(float3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }

__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }  // (torch.max propagates NaN)

// one wavefront per node of either cloud (two patch slots per lane): (transformed) node, |node|^2, max patch radius;
// also zeroes the counters
__global__ __launch_bounds__(256) void gt_prep_kernel(GtArgs a) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;  // wave-uniform
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.counts[0] = 0;
    a.counts[1] = 0;
  }
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.cnt[0]; i += blockDim.x) a.row_count[i] = 0;
  if (g >= a.cnt[0] + a.cnt[1]) return;
  const int c = g < a.cnt[0] ? 0 : 1;
  const int u = c == 0 ? g : g - a.cnt[0];
  const float* nd = a.nodes[c] + 3 * u;
  float3 node = make_float3(nd[0], nd[1], nd[2]);
  if (c == 1) node = transform_point(a.T, node);
  float best = 0.f;  // (every value is >= 0; masked slots count as 0)
  for (int s = lane; s < a.k; s += 64) {
    if (!slot_valid(a, c, u, s)) continue;
    const float3 p = slot_point(a, c, u, s);
    best = max_nan(best, sqrtf(sq_norm(make_float3(p.x - node.x, p.y - node.y, p.z - node.z))));
  }
  for (int off = 32; off > 0; off >>= 1) best = max_nan(best, __shfl_xor(best, off));  // (max: order-free)
  if (lane == 0) {
    a.node4[c][u] = make_float4(node.x, node.y, node.z, sq_norm(node));
    a.rad[c][u] = best;
  }
}

// one wavefront per (ref, src) node pair, grid-stride; blockDim = 64 so __syncthreads is the wave's own barrier
__global__ __launch_bounds__(64) void gt_pair_kernel(GtArgs a) {
  __shared__ float4 sp[kMaxK];
  const int lane = threadIdx.x;
  const int m = a.cnt[0], n = a.cnt[1];
  const int64_t total = static_cast<int64_t>(m) * n;
  for (int64_t p = blockIdx.x; p < total; p += gridDim.x) {
    const int i = static_cast<int>(p / n), j = static_cast<int>(p - static_cast<int64_t>(i) * n);
    const float4 x = a.node4[0][i], y = a.node4[1][j];
    const float dist = sqrtf(ref_sq_dist(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w));
    const bool masked = (a.node_mask[0] && !a.node_mask[0][i]) || (a.node_mask[1] && !a.node_mask[1][j]);
    if (masked || !(((a.rad[0][i] + a.rad[1][j]) + a.radius) - dist > 0.f)) {  // wave-uniform
      if (lane == 0) a.ov[p] = 0.f;
      continue;
    }
    if (lane == 0) atomicAdd(&a.counts[1], 1);
    // src patch -> LDS (w = |y|^2; invalid slots are skipped through the ballot mask)
    bool sv[2], rv[2];
    float4 rp[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int s = lane + 64 * h;
      sv[h] = s < a.k && slot_valid(a, 1, j, s);
      rv[h] = s < a.k && slot_valid(a, 0, i, s);
      if (s < a.k) {
        const float3 q = slot_point(a, 1, j, s);
        sp[s] = make_float4(q.x, q.y, q.z, sq_norm(q));
        const float3 r = slot_point(a, 0, i, s);
        rp[h] = make_float4(r.x, r.y, r.z, sq_norm(r));
      }
    }
    const unsigned long long sv_lo = __ballot(sv[0]), sv_hi = __ballot(sv[1]);
    const int n_ref = __popcll(__ballot(rv[0])) + __popcll(__ballot(rv[1]));
    const int n_src = __popcll(sv_lo) + __popcll(sv_hi);
    __syncthreads();
    bool hit[2] = {false, false};
    int src_hits = 0;
    for (int s = 0; s < a.k; ++s) {
      const unsigned long long word = s < 64 ? sv_lo : sv_hi;
      if (!((word >> (s & 63)) & 1ull)) continue;  // wave-uniform
      const float4 q = sp[s];                      // broadcast read
      bool any = false;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool t = rv[h] && ref_sq_dist(rp[h].x, rp[h].y, rp[h].z, rp[h].w, q.x, q.y, q.z, q.w) < a.r2;
        hit[h] = hit[h] || t;
        any = any || t;
      }
      src_hits += __ballot(any) != 0ull ? 1 : 0;
    }
    const int ref_hits = __popcll(__ballot(hit[0])) + __popcll(__ballot(hit[1]));
    if (lane == 0) {
      const float ro = static_cast<float>(ref_hits) / static_cast<float>(n_ref);
      const float so = static_cast<float>(src_hits) / static_cast<float>(n_src);
      const float o = (ro + so) / 2.f;
      a.ov[p] = o;
      if (o > 0.f) atomicAdd(&a.row_count[i], 1);
    }
    __syncthreads();  // (the next pair rewrites sp)
  }
}

// ordered compaction of ov > 0 (row-major = torch.nonzero's order): one workgroup per ref row i; its first output slot is
// the sum of the rows before it (row_count, from gt_pair_kernel), the order inside the row a ballot prefix per 256 columns
constexpr int kCompact = 256;
__global__ __launch_bounds__(kCompact) void gt_compact_kernel(const float* ov, const int32_t* row_count, int m, int n,
                                                              int64_t* out_idx, float* out_ov, int64_t capacity, int32_t* counts,
                                                              int32_t* status, int32_t* mirror) {
  __shared__ int64_t red[kCompact / 64];
  __shared__ int wave_tot[kCompact / 64];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int64_t before = 0;
  for (int r = t; r < i; r += kCompact) before += row_count[r];
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
  if (lane == 0) red[w] = before;
  __syncthreads();
  int64_t pos = 0;
  for (int v = 0; v < kCompact / 64; ++v) pos += red[v];
  const float* row = ov + static_cast<int64_t>(i) * n;
  for (int j0 = 0; j0 < n; j0 += kCompact) {  // (block-uniform loop)
    const int j = j0 + t;
    const float v = j < n ? row[j] : 0.f;
    const bool keep = v > 0.f;
    const unsigned long long bal = __ballot(keep);
    __syncthreads();  // (wave_tot of the previous tile has been read)
    if (lane == 0) wave_tot[w] = __popcll(bal);
    __syncthreads();
    int64_t q = pos + __popcll(bal & ((1ull << lane) - 1ull));
    for (int x = 0; x < w; ++x) q += wave_tot[x];
    if (keep && q < capacity) {
      out_idx[2 * q] = i;
      out_idx[2 * q + 1] = j;
      out_ov[q] = v;
    }
    for (int x = 0; x < kCompact / 64; ++x) pos += wave_tot[x];
  }
  if (i == m - 1 && t == 0) {  // pos = C
    counts[0] = static_cast<int32_t>(pos);
    if (pos > capacity && status) *status = 1;
    if (mirror) {
      mirror[0] = static_cast<int32_t>(pos);
      mirror[1] = counts[1];
    }
  }
}

struct GtWs {
  float4* node4[2];
  float* rad[2];
  float* ov;
  int32_t* row_count;
};

GtWs carve(Arena& ar, int64_t m, int64_t n) {
  GtWs w;
  w.node4[0] = ar.take<float4>(m);
  w.node4[1] = ar.take<float4>(n);
  w.rad[0] = ar.take<float>(m);
  w.rad[1] = ar.take<float>(n);
  w.ov = ar.take<float>(m * n);
  w.row_count = ar.take<int32_t>(m);
  return w;
}

}  // namespace

namespace rdm {

// shared by rdm_gt_node_correspondences and the engine entry (engine.hip); `mirror` (nullable): device address of mapped
// host memory that receives {C, B}
int gt_node_correspondences_impl(const float* ref_nodes, int64_t m, const float* src_nodes, int64_t n, const float* ref_points,
                                 const int64_t* ref_idx, int64_t ref_n_points, const float* src_points, const int64_t* src_idx,
                                 int64_t src_n_points, int k, const uint8_t* ref_node_mask, const uint8_t* src_node_mask,
                                 const uint8_t* ref_knn_mask, const uint8_t* src_knn_mask, const float* transform,
                                 double pos_radius, int64_t* out_indices, float* out_overlaps, int64_t capacity, int32_t* counts,
                                 int32_t* status, int32_t* mirror, void* ws, size_t ws_bytes, void* stream) {
  RDM_REQUIRE(ref_nodes && src_nodes && ref_points && src_points && transform && counts && (capacity == 0 || (out_indices && out_overlaps)),
              "rdm_gt_node_correspondences: null pointer");
  RDM_REQUIRE(m > 0 && n > 0 && k > 0 && k <= kMaxK && capacity >= 0 && m <= (int64_t(1) << 20) && n <= (int64_t(1) << 20) &&
                  m * n <= (int64_t(1) << 31),
              "rdm_gt_node_correspondences: bad sizes (m=%lld n=%lld k=%d capacity=%lld; k <= 128, m*n <= 2^31)", (long long)m,
              (long long)n, k, (long long)capacity);
  RDM_REQUIRE((ref_idx == nullptr || ref_n_points > 0) && (src_idx == nullptr || src_n_points > 0),
              "rdm_gt_node_correspondences: indexed patches need the cloud's point count");
  Arena ar(ws, ws_bytes);
  GtWs w = carve(ar, m, n);
  if (!ar.ok) {
    set_error("rdm_gt_node_correspondences: workspace too small (%zu < %zu)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  GtArgs a;
  a.nodes[0] = ref_nodes; a.nodes[1] = src_nodes;
  a.pts[0] = ref_points; a.pts[1] = src_points;
  a.idx[0] = ref_idx; a.idx[1] = src_idx;
  a.n_pts[0] = ref_n_points; a.n_pts[1] = src_n_points;
  a.node_mask[0] = ref_node_mask; a.node_mask[1] = src_node_mask;
  a.knn_mask[0] = ref_knn_mask; a.knn_mask[1] = src_knn_mask;
  a.cnt[0] = static_cast<int>(m); a.cnt[1] = static_cast<int>(n);
  a.k = k;
  a.T = transform;
  a.radius = static_cast<float>(pos_radius);
  a.r2 = static_cast<float>(pos_radius * pos_radius);  // (python: pos_radius ** 2 in double, compared in fp32)
  a.node4[0] = w.node4[0]; a.node4[1] = w.node4[1];
  a.rad[0] = w.rad[0]; a.rad[1] = w.rad[1];
  a.ov = w.ov;
  a.row_count = w.row_count;
  a.counts = counts;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t total = m * n;
  hipLaunchKernelGGL(gt_prep_kernel, dim3(static_cast<unsigned>(ceil_div<int64_t>(m + n, 4))), dim3(256), 0, st, a);
  hipLaunchKernelGGL(gt_pair_kernel, dim3(static_cast<unsigned>(total < 65536 ? total : 65536)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(gt_compact_kernel, dim3(static_cast<unsigned>(m)), dim3(kCompact), 0, st, w.ov, w.row_count, static_cast<int>(m),
                     static_cast<int>(n), out_indices, out_overlaps, capacity, counts, status, mirror);
  return launch_status("gt_node_correspondences kernels");
}

}  // namespace rdm

extern "C" size_t rdm_gt_node_correspondences_workspace_bytes(int64_t m, int64_t n) {
  rdm::Arena a(nullptr, 0);
  carve(a, m > 0 ? m : 1, n > 0 ? n : 1);
  return a.off;
}

extern "C" int rdm_gt_node_correspondences(const float* ref_nodes, int64_t m, const float* src_nodes, int64_t n,
                                           const float* ref_points, const int64_t* ref_knn_idx, int64_t ref_n_points,
                                           const float* src_points, const int64_t* src_knn_idx, int64_t src_n_points, int k,
                                           const uint8_t* ref_node_mask, const uint8_t* src_node_mask,
                                           const uint8_t* ref_knn_mask, const uint8_t* src_knn_mask, const float* transform,
                                           double pos_radius, int64_t* out_indices, float* out_overlaps, int64_t capacity,
                                           int32_t* counts, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  RDM_REQUIRE(status, "rdm_gt_node_correspondences: null status");
  return rdm::gt_node_correspondences_impl(ref_nodes, m, src_nodes, n, ref_points, ref_knn_idx, ref_n_points, src_points,
                                           src_knn_idx, src_n_points, k, ref_node_mask, src_node_mask, ref_knn_mask, src_knn_mask,
                                           transform, pos_radius, out_indices, out_overlaps, capacity, counts, status, nullptr,
                                           ws, ws_bytes, stream);
}
