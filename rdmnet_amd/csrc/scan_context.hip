// Loop-closure detection: Scan Context place descriptors (Kim & Kim, IROS 2018) and the exhaustive search over them
// (include/rdmnet_hip.h, "scan context").  The project's own definition, pinned to the float64
// restatement tests/scan_context_restatement.py.
//
// Descriptor: a scan's points are split over kSplits workgroups; each keeps the n_rings x n_sectors bins in LDS as
// order-preserving integer keys of the fp32 value z + lidar_height (0 = no point) under an integer atomic max, so that the
// result does not depend on the order of the points; a second launch merges the splits (again a max), decodes the keys and
// writes the descriptor, its column-normalised form and the valid-column mask.  The bin of a point is computed in float64
// with the restatement's expressions.
//
// Distance: sum_n(Q, C) = sum over rings r and columns j of Qn[r, j] Cn[r, (j - n) mod n_sectors] on the column-normalised
// descriptors.  Lane = shift n.  A wave keeps, for kTC candidates and one ring, the candidate's ring row as seen under ITS
// shift in registers (kTC x 64 VGPRs, read from a twice-repeated copy of the row in LDS: lane n reads k = j - n + n_sectors),
// and sweeps a block of kQB queries whose values are wave-uniform: they come through the scalar cache as SGPR operands of
// the FMAs, so the inner loop is one v_fma per product with neither an LDS nor a vector-memory read beside it.  Rows are padded
// to 64 columns with zeros, which is what lets one kernel serve every n_sectors <= 64 (60 of 64 lanes and 60 of 64 FMAs are
// useful at the default).  A ring's sum is formed on its own and then added to the pair's total, so that the 64 products of
// a ring are added at the magnitude of one ring and not of the whole sum.  The minimum over shifts is a wave reduction;
// per-query results of the candidate tiles meet in one 64-bit integer atomic min per query (distance key, candidate,
// shift), which is order independent and gives the lowest candidate among equal distances.
#include <cmath>

#include "../../include/rdmnet_hip.h"
#include "common.h"

namespace rdm {
namespace {

constexpr int kMaxDim = RDM_SCAN_CONTEXT_MAX_DIM;  // n_rings, n_sectors <= 64
constexpr int kLd = RDM_SCAN_CONTEXT_LD;           // columns of a row of the normalised form
constexpr int kBins = kMaxDim * kMaxDim;
constexpr int kSplits = 8;     // workgroups a scan's points are split over
constexpr int kBinBlock = 256;
constexpr int kQB = 16;        // queries a wave sweeps per candidate group
constexpr int kTC = 2;         // candidates a wave holds in registers
constexpr int kWaves = 4;      // waves of a distance workgroup
constexpr int kCT = kWaves * kTC;  // candidates of a distance workgroup
constexpr int kRow = 2 * kMaxDim;  // floats of a staged candidate row: the row twice, then zeros
constexpr int kIndexBits = 26, kShiftBits = 6;
constexpr int64_t kMaxCandidates = int64_t(1) << kIndexBits;
static_assert(kLd == kMaxDim && kMaxDim == kWave, "lane = shift and one zero-padded row per ring");

__device__ __forceinline__ bool valid_dims(int n_rings, int n_sectors) {
  return n_rings >= 1 && n_rings <= kMaxDim && n_sectors >= 1 && n_sectors <= kMaxDim;
}

// ---- descriptor ---------------------------------------------------------------------------------------------------------------

// grid (kSplits, n_scans): partial[scan][split][n_rings * n_sectors] keys
__global__ void __launch_bounds__(kBinBlock) bin_kernel(const float* __restrict__ points, long long ld, long long n_points,
                                                        const int64_t* __restrict__ offsets, int n_rings, int n_sectors,
                                                        double max_range, float lidar_height, uint32_t* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ uint32_t bins[kBins];
  if (!valid_dims(n_rings, n_sectors)) return;
  const int nb = n_rings * n_sectors;
  for (int b = threadIdx.x; b < nb; b += kBinBlock) bins[b] = 0u;
  __syncthreads();
  const long long scan = blockIdx.y;
  long long begin = offsets[scan], end = offsets[scan + 1];
  begin = begin < 0 ? 0 : begin;
  end = end > n_points ? n_points : end;  // (a bad offsets array reads nothing outside the cloud)
  const long long n = end > begin ? end - begin : 0;
  const long long chunk = (n + kSplits - 1) / kSplits;
  const long long lo = begin + static_cast<long long>(blockIdx.x) * chunk;
  long long hi = lo + chunk;
  hi = hi > begin + n ? begin + n : hi;
  const double two_pi = 6.283185307179586476925286766559;
  for (long long i = lo + threadIdx.x; i < hi; i += kBinBlock) {
    const float* p = points + i * ld;
    const float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    const double xd = x, yd = y;
    const double r = sqrt(xd * xd + yd * yd);
    if (r == 0.0 || r > max_range) continue;
    int ring = static_cast<int>(floor(r / max_range * n_rings));
    ring = ring > n_rings - 1 ? n_rings - 1 : (ring < 0 ? 0 : ring);
    double th = atan2(yd, xd);
    if (th < 0.0) th += two_pi;
    int sec = static_cast<int>(floor(th / two_pi * n_sectors));
    sec = sec > n_sectors - 1 ? n_sectors - 1 : (sec < 0 ? 0 : sec);
    atomicMax(&bins[ring * n_sectors + sec], order_key(z + lidar_height));
  }
  __syncthreads();
  uint32_t* out = partial + (scan * kSplits + blockIdx.x) * static_cast<long long>(nb);
  for (int b = threadIdx.x; b < nb; b += kBinBlock) out[b] = bins[b];
}

// Column norms of one descriptor held in LDS (d[n_rings * n_sectors]) -> normalised form [n_rings][kLd] (0 in invalid and pad
// columns) and the valid-column mask.  Float64 sums of the fp32 squares, one rounding of the quotient.
__device__ void normalise_columns(const float* d, int n_rings, int n_sectors, float* __restrict__ norm, uint64_t* __restrict__ valid,
                                  double* inv, unsigned long long* mask) {
  const int t = threadIdx.x;
  if (t == 0) *mask = 0ull;
  __syncthreads();
  if (t < kLd) {
    double s = 0.0;
    if (t < n_sectors)
      for (int r = 0; r < n_rings; ++r) {
        const double v = d[r * n_sectors + t];
        s += v * v;
      }
    const bool ok = s > 0.0;
    inv[t] = ok ? sqrt(s) : 0.0;
    if (ok) atomicOr(mask, 1ull << t);
  }
  __syncthreads();
  for (int e = t; e < n_rings * kLd; e += blockDim.x) {
    const int r = e / kLd, j = e % kLd;
    float v = 0.f;
    if (j < n_sectors && inv[j] > 0.0) v = static_cast<float>(static_cast<double>(d[r * n_sectors + j]) / inv[j]);
    norm[e] = v;
  }
  if (t == 0) *valid = *mask;
}

// grid (n_scans): max over the splits, decode, write desc / norm / valid (each optional)
__global__ void __launch_bounds__(kBinBlock) merge_kernel(const uint32_t* __restrict__ partial, int n_rings, int n_sectors,
                                                          float* __restrict__ desc, float* __restrict__ norm,
                                                          uint64_t* __restrict__ valid) {
  __shared__ float d[kBins];
  __shared__ double inv[kLd];
  __shared__ unsigned long long mask;
  if (!valid_dims(n_rings, n_sectors)) return;
  const int nb = n_rings * n_sectors;
  const long long scan = blockIdx.x;
  for (int b = threadIdx.x; b < nb; b += kBinBlock) {
    uint32_t k = 0u;
    for (int s = 0; s < kSplits; ++s) {
      const uint32_t v = partial[(scan * kSplits + s) * static_cast<long long>(nb) + b];
      k = v > k ? v : k;
    }
    const float v = k == 0u ? 0.f : key_value(k);
    d[b] = v;
    if (desc) desc[scan * nb + b] = v;
  }
  __syncthreads();
  if (norm && valid) normalise_columns(d, n_rings, n_sectors, norm + scan * static_cast<long long>(n_rings) * kLd, valid + scan, inv, &mask);
}

// grid (n_scans): raw descriptors -> norm / valid (the distance call's own preparation)
__global__ void __launch_bounds__(kBinBlock) normalise_kernel(const float* __restrict__ desc, int n_rings, int n_sectors,
                                                              float* __restrict__ norm, uint64_t* __restrict__ valid) {
  __shared__ float d[kBins];
  __shared__ double inv[kLd];
  __shared__ unsigned long long mask;
  if (!valid_dims(n_rings, n_sectors)) return;
  const int nb = n_rings * n_sectors;
  const long long scan = blockIdx.x;
  for (int b = threadIdx.x; b < nb; b += kBinBlock) d[b] = desc[scan * nb + b];
  __syncthreads();
  normalise_columns(d, n_rings, n_sectors, norm + scan * static_cast<long long>(n_rings) * kLd, valid + scan, inv, &mask);
}

// ---- distance and search ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// columns valid on both sides under shift n: query column j against candidate column (j - n) mod n_sectors
__device__ __forceinline__ int both_valid(uint64_t vq, uint64_t vc, int n, int n_sectors) {
  const uint64_t all = n_sectors == 64 ? ~0ull : ((1ull << n_sectors) - 1ull);
  const uint64_t rot = n == 0 ? vc : (((vc << n) | (vc >> (n_sectors - n))) & all);
  return __popcll(vq & rot);
}

// grid (ceil(n_c / kCT), ceil(n_q / kQB)), kWaves * 64 threads.  qn / cn: normalised forms [n][n_rings][kLd].
// best: one key per query, preset to all ones; dist / shift: optional full matrices [n_q][n_c].
__global__ void __launch_bounds__(kWaves* kWave) distance_kernel(const float* __restrict__ qn, const uint64_t* __restrict__ qvalid,
                                                                 long long n_q, const float* __restrict__ cn,
                                                                 const uint64_t* __restrict__ cvalid, long long n_c, int n_rings,
                                                                 int n_sectors, long long q_base, long long c_base,
                                                                 long long exclude_recent, unsigned long long* __restrict__ best,
                                                                 float* __restrict__ dist, int32_t* __restrict__ shift) {
  __shared__ float rows[2][kCT][kRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long q0 = static_cast<long long>(blockIdx.y) * kQB, c0 = static_cast<long long>(blockIdx.x) * kCT;
  const bool window = exclude_recent >= 0;
  // best-only mode: a tile without an eligible pair has nothing to add (the most eligible pair is the last query with the
  // first candidate of the tile)
  if (dist == nullptr && window) {
    const long long q_last = (q0 + kQB - 1 < n_q - 1 ? q0 + kQB - 1 : n_q - 1) + q_base;
    if (q_last - (c0 + c_base) < exclude_recent) return;
  }
  for (int e = tid; e < 2 * kCT * kRow; e += kWaves * kWave) (&rows[0][0][0])[e] = 0.f;
  __syncthreads();

  // staging: thread -> (candidate of the tile, column), kCT * 64 = 2 elements per thread and ring
  const int n = lane < n_sectors ? lane : 0;  // lanes beyond the last shift compute shift 0 and drop it
  float tot[kQB][kTC];
#pragma unroll
  for (int q = 0; q < kQB; ++q)
#pragma unroll
    for (int t = 0; t < kTC; ++t) tot[q][t] = 0.f;

  for (int r = 0; r < n_rings; ++r) {
    float(*buf)[kRow] = rows[r & 1];
    for (int e = tid; e < kCT * kLd; e += kWaves * kWave) {
      const int c = e / kLd, j = e % kLd;
      if (j < n_sectors) {
        const long long cg = c0 + c;
        const float v = cg < n_c ? cn[(cg * n_rings + r) * kLd + j] : 0.f;
        buf[c][j] = v;
        buf[c][j + n_sectors] = v;
      }
    }
    __syncthreads();  // (one barrier per ring: the next ring writes the other buffer)
    float creg[kTC][kLd];
#pragma unroll
    for (int t = 0; t < kTC; ++t)
#pragma unroll
      for (int j = 0; j < kLd; ++j) creg[t][j] = buf[wave * kTC + t][j - n + n_sectors];  // k in [1, 63 + n_sectors]
#pragma unroll
    for (int q = 0; q < kQB; ++q) {
      long long qg = q0 + q;
      qg = qg < n_q ? qg : n_q - 1;
      const float* __restrict__ qrow = qn + (qg * n_rings + r) * kLd;  // wave-uniform: scalar loads
      float part[kTC];
#pragma unroll
      for (int t = 0; t < kTC; ++t) part[t] = 0.f;
#pragma unroll
      for (int j = 0; j < kLd; ++j) {
        const float s = qrow[j];
#pragma unroll
        for (int t = 0; t < kTC; ++t) part[t] = fmaf(s, creg[t][j], part[t]);
      }
#pragma unroll
      for (int t = 0; t < kTC; ++t) tot[q][t] += part[t];
    }
  }

  // per (query, candidate): d_n in lane n, minimum over the lanes with the lowest n among equals
  unsigned long long mine = ~0ull;  // lane q keeps the key of query q0 + q over this wave's candidates
#pragma unroll
  for (int t = 0; t < kTC; ++t) {
    const long long cg = c0 + wave * kTC + t;
    const bool c_ok = cg < n_c;
    const uint64_t vc = cvalid[c_ok ? cg : n_c - 1];
#pragma unroll
    for (int q = 0; q < kQB; ++q) {
      const long long qg = q0 + q;
      const bool q_ok = qg < n_q;
      const uint64_t vq = qvalid[q_ok ? qg : n_q - 1];
      const int cnt = both_valid(vq, vc, n, n_sectors);
      const float d = cnt > 0 ? 1.f - tot[q][t] / static_cast<float>(cnt) : 1.f;
      unsigned long long key = lane < n_sectors ? (static_cast<unsigned long long>(order_key(d)) << 32) | static_cast<unsigned>(lane)
                                                : ~0ull;
      key = wave_min_u64(key);
      if (lane == q && q_ok && c_ok) {
        const float dmin = key_value(static_cast<uint32_t>(key >> 32));
        const int smin = static_cast<int>(key & 63ull);
        if (dist) {
          dist[qg * n_c + cg] = dmin;
          shift[qg * n_c + cg] = smin;
        }
        if (!window || (qg + q_base) - (cg + c_base) >= exclude_recent) {
          const unsigned long long k = (key & 0xffffffff00000000ull) | (static_cast<unsigned long long>(cg) << kShiftBits) |
                                       static_cast<unsigned long long>(smin);
          mine = k < mine ? k : mine;
        }
      }
    }
  }
  if (lane < kQB && mine != ~0ull) atomicMin(best + q0 + lane, mine);
}

__global__ void best_kernel(const unsigned long long* __restrict__ best, long long n_q, float* __restrict__ distance,
                            int32_t* __restrict__ index, int32_t* __restrict__ shift) {
  const long long q = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  if (q >= n_q) return;
  const unsigned long long k = best[q];
  const bool none = k == ~0ull;
  distance[q] = none ? INFINITY : key_value(static_cast<uint32_t>(k >> 32));
  index[q] = none ? -1 : static_cast<int32_t>((k >> kShiftBits) & ((1ull << kIndexBits) - 1ull));
  shift[q] = none ? -1 : static_cast<int32_t>(k & ((1ull << kShiftBits) - 1ull));
}

bool dims_ok(int n_rings, int n_sectors) {
  return n_rings >= 1 && n_rings <= kMaxDim && n_sectors >= 1 && n_sectors <= kMaxDim;
}

struct DistWork {
  float *qn, *cn;
  uint64_t *qvalid, *cvalid;
  unsigned long long* best;
};

bool carve(Arena& ar, int64_t n_q, int64_t n_c, int n_rings, DistWork& w) {
  const size_t q = static_cast<size_t>(n_q > 0 ? n_q : 1), c = static_cast<size_t>(n_c > 0 ? n_c : 1);
  w.qn = ar.take<float>(q * n_rings * kLd);
  w.qvalid = ar.take<uint64_t>(q);
  w.cn = ar.take<float>(c * n_rings * kLd);
  w.cvalid = ar.take<uint64_t>(c);
  w.best = ar.take<unsigned long long>(q);
  return ar.ok;
}

}  // namespace
}  // namespace rdm

extern "C" size_t rdm_scan_context_workspace_bytes(int64_t n_scans, int n_rings, int n_sectors) {
  using namespace rdm;
  if (n_scans < 0 || !dims_ok(n_rings, n_sectors)) return 0;
  Arena ar(nullptr, 0);
  ar.take<uint32_t>(static_cast<size_t>(n_scans > 0 ? n_scans : 1) * kSplits * n_rings * n_sectors);
  return ar.off;
}

extern "C" int rdm_scan_context(const float* points, int64_t ld, int64_t n_points, const int64_t* offsets, int64_t n_scans,
                                int n_rings, int n_sectors, double max_range, double lidar_height, float* desc, float* desc_norm,
                                uint64_t* valid, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(dims_ok(n_rings, n_sectors), "rdm_scan_context: n_rings and n_sectors must be 1 ... %d, got %d and %d", kMaxDim, n_rings,
              n_sectors);
  RDM_REQUIRE(n_scans >= 0 && n_scans <= 65535 && n_points >= 0 && ld >= 3, "rdm_scan_context: bad sizes (at most 65535 scans a call)");
  RDM_REQUIRE(max_range > 0.0 && std::isfinite(max_range) && std::isfinite(lidar_height), "rdm_scan_context: bad max_range or lidar_height");
  RDM_REQUIRE((desc_norm == nullptr) == (valid == nullptr), "rdm_scan_context: desc_norm and valid go together");
  if (n_scans == 0) return RDM_OK;
  RDM_REQUIRE(offsets && (points || n_points == 0) && (desc || desc_norm), "rdm_scan_context: null argument");
  Arena ar(ws, ws_bytes);
  uint32_t* partial = ar.take<uint32_t>(static_cast<size_t>(n_scans) * kSplits * n_rings * n_sectors);
  if (!ar.ok) {
    set_error("rdm_scan_context: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bin_kernel, dim3(kSplits, static_cast<unsigned>(n_scans)), dim3(kBinBlock), 0, s, points, static_cast<long long>(ld),
                     static_cast<long long>(n_points), offsets, n_rings, n_sectors, max_range, static_cast<float>(lidar_height), partial);
  hipLaunchKernelGGL(merge_kernel, dim3(static_cast<unsigned>(n_scans)), dim3(kBinBlock), 0, s, partial, n_rings, n_sectors, desc,
                     desc_norm, valid);
  return launch_status("rdm_scan_context");
}

extern "C" size_t rdm_scan_context_distance_workspace_bytes(int64_t n_q, int64_t n_c, int n_rings, int n_sectors) {
  using namespace rdm;
  if (n_q < 0 || n_c < 0 || n_c > kMaxCandidates || !dims_ok(n_rings, n_sectors)) return 0;
  Arena ar(nullptr, 0);
  DistWork w;
  carve(ar, n_q, n_c, n_rings, w);
  return ar.off;
}

extern "C" int rdm_scan_context_distance(const float* q_desc, int64_t n_q, const float* c_desc, int64_t n_c, int n_rings,
                                         int n_sectors, int64_t q_base, int64_t c_base, int64_t exclude_recent,
                                         float* best_distance, int32_t* best_index, int32_t* best_shift, float* dist,
                                         int32_t* shift, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(dims_ok(n_rings, n_sectors), "rdm_scan_context_distance: n_rings and n_sectors must be 1 ... %d, got %d and %d", kMaxDim,
              n_rings, n_sectors);
  RDM_REQUIRE(n_q >= 0 && n_c >= 0, "rdm_scan_context_distance: negative size");
  if (n_c > kMaxCandidates) {
    set_error("rdm_scan_context_distance: %lld candidates, a call takes at most %lld", static_cast<long long>(n_c),
              static_cast<long long>(kMaxCandidates));
    return RDM_ERR_CAPACITY;
  }
  RDM_REQUIRE((dist == nullptr) == (shift == nullptr), "rdm_scan_context_distance: dist and shift go together");
  if (n_q == 0) return RDM_OK;
  RDM_REQUIRE(q_desc && (c_desc || n_c == 0) && best_distance && best_index && best_shift, "rdm_scan_context_distance: null argument");
  const int64_t q_tiles = ceil_div<int64_t>(n_q, kQB), c_tiles = ceil_div<int64_t>(n_c, kCT);
  RDM_REQUIRE(q_tiles <= 65535, "rdm_scan_context_distance: at most %d queries a call", 65535 * kQB);
  Arena ar(ws, ws_bytes);
  DistWork w;
  if (!carve(ar, n_q, n_c, n_rings, w)) {
    set_error("rdm_scan_context_distance: workspace too small (%zu < %zu bytes)", ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(normalise_kernel, dim3(static_cast<unsigned>(n_q)), dim3(kBinBlock), 0, s, q_desc, n_rings, n_sectors, w.qn, w.qvalid);
  const bool same = q_desc == c_desc && n_q == n_c;  // a sequence against itself: one normalised copy
  if (same) {
    w.cn = w.qn;
    w.cvalid = w.qvalid;
  } else if (n_c > 0) {
    hipLaunchKernelGGL(normalise_kernel, dim3(static_cast<unsigned>(n_c)), dim3(kBinBlock), 0, s, c_desc, n_rings, n_sectors, w.cn,
                       w.cvalid);
  }
  fill_words<unsigned long long>(w.best, n_q, ~0ull, s);
  if (n_c > 0)
    hipLaunchKernelGGL(distance_kernel, dim3(static_cast<unsigned>(c_tiles), static_cast<unsigned>(q_tiles)), dim3(kWaves * kWave), 0, s,
                       w.qn, w.qvalid, static_cast<long long>(n_q), w.cn, w.cvalid, static_cast<long long>(n_c), n_rings, n_sectors,
                       static_cast<long long>(q_base), static_cast<long long>(c_base), static_cast<long long>(exclude_recent), w.best,
                       dist, shift);
  hipLaunchKernelGGL(best_kernel, dim3(static_cast<unsigned>(ceil_div<int64_t>(n_q, 256))), dim3(256), 0, s, w.best,
                     static_cast<long long>(n_q), best_distance, best_index, best_shift);
  return launch_status("rdm_scan_context_distance");
}
