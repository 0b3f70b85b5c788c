// Voxel map: the scans of a sequence fused under its trajectory into one persistent hash table in world coordinates
// (include/rdmnet_hip.h, "voxel map").  The project's own definition, pinned bit for bit to the NumPy
// restatement tests/voxel_map_restatement.py.
//
// Table: open addressing with linear probing over a power-of-two number of slots, structure of arrays behind a block of six
// uint64 counters: keys uint64 [S] (all ones = empty), counts uint32 [S], C planes of int64 sums [C][S]; 12 + 8 C bytes a slot.
// A key is the three cells + 2^20 at 21 bits each, so it never equals the empty word.  Slots only ever go from empty to a key
// (one 64-bit compare-and-swap), which is what makes the lock-free insert exact: the first slot of a key's probe sequence that
// is empty or holds the key is the same for every thread that looks for it, whenever it looks.
//
// Integrate: one thread per point.  The point's scan is found by a bisection of the offsets (17 steps at 65 536 scans), the
// pose is read from the device, the transform and the quantisation are float64 with the restatement's association and no
// contraction, and the point lands in its voxel as one uint32 and C int64 atomic adds of fixed-point values: integer sums are
// associative, so the map depends on the set of points and on nothing else.  No merge of equal keys inside a wavefront
// before the atomics: the plain form is the one that was measured (docs/EXPERIMENTS.md).  The probe is bounded by the capacity;
// a point that finds neither its key nor an empty slot in one full cycle is counted in dropped_full and touches nothing.
//
// Extract: slot -> (key or all ones, slot), one radix sort of the S pairs (the unselected sort to the end; no read-back of
// the count is needed before the sort), then one thread per selected row.
//
// Moments (include/rdmnet_hip.h, "voxel moments"; tests/voxel_moments_restatement.py): a second caller-owned block of nine int64
// sums per slot, addressed by the map's slot index -- the first and second moments of the 12-bit local coordinates u_d, so every
// voxel gets a mean, a covariance and a normal.  integrate_kernel<true, .> is the integrate kernel with nine more integer adds into
// the slot that find_or_claim returned; integrate_kernel<false, false>, the plain one, is the same body with that block compiled out.  Extraction shares the
// selection and the sort and solves the 3 x 3 symmetric eigenproblem per row with a float64 cyclic Jacobi of kSweeps sweeps.
//
// Observations (include/rdmnet_hip.h, "voxel observations"; tests/voxel_observations_restatement.py): a third caller-owned block,
// addressed by the map's slot index -- per slot a 64-bit scratch mask and the record {scans, first, last}: in how many distinct scans
// the voxel was seen, and the smallest and the largest of their ids.  integrate_kernel<., true> is the integrate kernel plus, after the
// point is counted, one load of the slot's mask and, where the scan's bit is still clear, one atomicOr; the one thread that got the
// bit clear back updates the record.  Bits only go from 0 to 1 inside a call, so a set bit seen by the plain load is final.
//
// Queries (include/rdmnet_hip.h, "voxel map queries"; tests/voxel_query_restatement.py): register's per-point lookup and distance, kept
// per point and not summed -- query_kernel, below the registration.  All three blocks are only read.
//
// State (include/rdmnet_hip.h, "voxel map state"; tests/voxel_state_restatement.py): export is a third emit kernel behind the extract
// driver that writes a row's integers as they stand in its slot; import is integrate with a record in the place of a point -- the same
// find_or_claim, the same integer atomic adds, the block's tallies through shared memory -- so a saved map reloads, and two maps of
// different scans add, to the bits of the map built in one pass.
//
// Alignment (include/rdmnet_hip.h, "voxel map alignment"; tests/voxel_align_restatement.py): register with another map's voxel records
// in the place of a scan's points -- accumulate_kernel with RecordRow where register has PointRow; the init and finalize kernels and
// the host's gauss_newton driver are shared.
//
// The pinned definitions are written once: the point gate (gate_sensor, gate_world over world_fixed; integrate, register and query;
// world_fixed alone: align's record), the key (pack_key, key_cell), the voxel Gaussian (voxel_gaussian over sum_mean and
// sums_covariance; both extracts, register, query, and align's record through the two parts), the visit of a cell and its six face
// neighbours (for_each_neighbor; register, align and query), the weight of a residual (voxel_precision) and a pair's sums (accumulate_pairs;
// register and align).  `#pragma clang fp contract(off)` is lexical and does not follow an inlined callee: every helper with pinned
// arithmetic opens with it itself, and jacobi3 and rodrigues, which stand outside any such block, stay there.
#include <cmath>
#include <string>

#include "../../include/rdmnet_hip.h"
#include "cell_index.h"
#include "common.h"

namespace rdm {
namespace {

constexpr int kFrac = RDM_VOXEL_MAP_FRAC_BITS;
constexpr int kMaxC = RDM_VOXEL_MAP_MAX_CHANNELS;
constexpr int kStats = RDM_VOXEL_MAP_STATS;
constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 1u << 20;  // the point and slot kernels stride over at most this many blocks
constexpr unsigned long long kEmpty = ~0ull;
constexpr long long kHalf = 1ll << 20;               // cells lie in [-2^20, 2^20)
constexpr double kScale = 1048576.0;                 // 2^kFrac
constexpr double kQLimit = 1099511627776.0;          // 2^40 = 2^20 cells of 2^20 steps
constexpr int64_t kMaxCapacity = int64_t(1) << 30;   // slots are sorted as int32 values under a 32-bit count
static_assert(kFrac == 20, "the key layout and kQLimit assume 20 fractional bits");
constexpr int kPlanes = RDM_VOXEL_MOMENTS_PLANES;   // u_x, u_y, u_z, then u_a u_b for ab = xx, xy, xz, yy, yz, zz
constexpr int kMomShift = RDM_VOXEL_MOMENTS_SHIFT;  // u_d = (Q_d - (cell_d << kFrac)) >> kMomShift: 12 bits
constexpr double kMomSteps = 4096.0;                // 2^(kFrac - kMomShift) steps of u_d per voxel edge
constexpr int kSweeps = 8;                          // cyclic Jacobi sweeps (a 3 x 3 symmetric matrix converges in 4 to 5)
static_assert(kPlanes == 9 && kFrac - kMomShift == 12, "nine sums of 12-bit local coordinates");
constexpr int kMaxObsScans = RDM_VOXEL_OBSERVATIONS_MAX_SCANS;  // scans of one integrate call: the bits of a slot's mask
constexpr int64_t kMaxScanId = 0x7fffffffll;                    // ids lie below this: `first` of a slot that observed nothing
static_assert(kMaxObsScans == 64, "one 64-bit mask per slot");

enum { kOccupied = 0, kIntegrated, kNonfinite, kRange, kExtent, kDropped };

struct Table {
  unsigned long long* counters;  // [kStats]
  unsigned long long* keys;      // [S]
  uint32_t* counts;              // [S]
  unsigned long long* sums;      // [C][S], two's-complement int64
};

bool shape_ok(int64_t capacity, int channels) {
  return capacity >= 64 && capacity <= kMaxCapacity && (capacity & (capacity - 1)) == 0 && channels >= 3 && channels <= kMaxC;
}

bool carve(Arena& ar, int64_t capacity, int channels, Table& t) {
  const size_t s = static_cast<size_t>(capacity);
  t.counters = ar.take<unsigned long long>(kStats);
  t.keys = ar.take<unsigned long long>(s);
  t.counts = ar.take<uint32_t>(s);
  t.sums = ar.take<unsigned long long>(s * channels);
  return ar.ok;
}

__device__ __forceinline__ unsigned long long mix(unsigned long long k) {  // the 64-bit finaliser of MurmurHash3
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The slot of `key`, claimed if it is new (*claimed = 1), or -1 after one full cycle without the key or an empty slot.
__device__ __forceinline__ long long find_or_claim(unsigned long long* __restrict__ keys, long long capacity, unsigned long long key,
                                                   int* claimed) {
  const unsigned long long mask = static_cast<unsigned long long>(capacity) - 1ull;
  unsigned long long slot = mix(key) & mask;
  *claimed = 0;
  for (long long probe = 0; probe < capacity; ++probe) {
    unsigned long long k = ld_agent(keys + slot);
    if (k == kEmpty) {
      k = atomicCAS(keys + slot, kEmpty, key);
      if (k == kEmpty) {
        *claimed = 1;
        return static_cast<long long>(slot);
      }
    }
    if (k == key) return static_cast<long long>(slot);
    slot = (slot + 1ull) & mask;
  }
  return -1;
}

// Sum k of a slot in the moments block.  Slot-major: a slot's nine sums are 72 consecutive bytes, so a point's nine adds fall
// into two (at most three) 64-byte lines.  -DRDM_VOXEL_MOMENTS_PLANE_MAJOR builds the [9][S] layout of the table's own sums, for the
// comparison in docs/EXPERIMENTS.md; nothing outside this function knows the layout.
__device__ __forceinline__ long long moment_at(long long slot, int k, long long capacity) {
#ifdef RDM_VOXEL_MOMENTS_PLANE_MAJOR
  return k * capacity + slot;
#else
  (void)capacity;
  return slot * kPlanes + k;
#endif
}

// The observations block: the masks as one plane (the sweep before a call and the one load a point are dense in it), then the records.
struct Observations {
  unsigned long long* mask;  // [S] scratch: bit s = scan s of the running call was seen
  int* record;               // [S] records, through observed_at only
};
enum { kObsScans = 0, kObsFirst, kObsLast, kObsFields };

bool carve_observations(Arena& ar, int64_t capacity, Observations& o) {
  const size_t s = static_cast<size_t>(capacity);
  o.mask = ar.take<unsigned long long>(s);
  o.record = ar.take<int>(s * kObsFields);
  return ar.ok;
}

// Field k of a slot's record.  Slot-major: the three fields are 12 consecutive bytes, so a first sighting's three atomics fall into
// one (at most two) 64-byte lines; nothing outside this function knows the layout.
__device__ __forceinline__ long long observed_at(long long slot, int k) { return slot * kObsFields + k; }

__global__ void __launch_bounds__(kBlock) reset_kernel(Table t, long long capacity, int channels) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (first < kStats) t.counters[first] = 0ull;
  for (long long i = first; i < capacity; i += stride) {
    t.keys[i] = kEmpty;
    t.counts[i] = 0u;
    for (int c = 0; c < channels; ++c) t.sums[c * capacity + i] = 0ull;
  }
}

// The key of a cell: the three cells + 2^20 at 21 bits each, x highest, so keys ascend with (cell x, cell y, cell z).
__device__ __forceinline__ unsigned long long pack_key(long long cx, long long cy, long long cz) {
  return (static_cast<unsigned long long>(cx + kHalf) << 42) | (static_cast<unsigned long long>(cy + kHalf) << 21) |
         static_cast<unsigned long long>(cz + kHalf);
}

__device__ __forceinline__ long long key_cell(unsigned long long key, int d) {
  return static_cast<long long>((key >> (21 * (2 - d))) & 0x1fffffull) - kHalf;
}

// The point gate of integrate and register, in two steps so that a row's pose can be looked up behind the sensor-frame verdicts.  A
// verdict is the counter that integrate tallies the row in.  Sensor frame: the row's values into v (zeros beyond `channels`) ->
// kNonfinite, kRange (lo2 <= |xyz|^2 <= hi2 fails) or kPass.
constexpr int kPass = kIntegrated;
__device__ __forceinline__ int gate_sensor(const float* __restrict__ p, int channels, double lo2, double hi2, float (&v)[kMaxC]) {
#pragma clang fp contract(off)
  bool finite = true;
  for (int c = 0; c < kMaxC; ++c) {
    v[c] = c < channels ? p[c] : 0.f;
    finite = finite && isfinite(v[c]);
  }
  if (!finite) return kNonfinite;
  const double x = v[0], y = v[1], z = v[2];
  const double r2 = (x * x + y * y) + z * z;
  return lo2 <= r2 && r2 <= hi2 ? kPass : kRange;
}

// wd = X (x, y, z) (X: the first 12 doubles of a row-major 4 x 4) with the restatement's association and q[0 .. 2] = its fixed-point
// coordinates on the grid of `voxel` (0 for a coordinate outside) -> whether all three cells lie in [-2^20, 2^20).
__device__ __forceinline__ bool world_fixed(const double* __restrict__ X, double x, double y, double z, double voxel, double (&wd)[3],
                                            long long* __restrict__ q) {
#pragma clang fp contract(off)
  bool inside = true;
  for (int d = 0; d < 3; ++d) {
    wd[d] = ((X[4 * d] * x + X[4 * d + 1] * y) + X[4 * d + 2] * z) + X[4 * d + 3];
    const double f = floor(wd[d] / voxel * kScale);
    const bool ok = f >= -kQLimit && f < kQLimit;  // (NaN and infinities fail)
    inside = inside && ok;
    q[d] = ok ? static_cast<long long>(f) : 0ll;
  }
  return inside;
}

// World frame, after kPass above: world_fixed of the row's xyz, then q[3 ..] = the fixed-point attributes (meaningful on kPass) ->
// kExtent (a cell outside [-2^20, 2^20) or |attribute| >= 2^20) or kPass.
__device__ __forceinline__ int gate_world(const float (&v)[kMaxC], const double* __restrict__ X, double voxel, double (&wd)[3],
                                          long long (&q)[kMaxC]) {
#pragma clang fp contract(off)
  bool inside = world_fixed(X, v[0], v[1], v[2], voxel, wd, q);
  for (int c = 3; c < kMaxC; ++c) {
    const double a = v[c];
    inside = inside && fabs(a) < kScale;
    q[c] = llrint(a * kScale);  // (finite)
  }
  return inside ? kPass : kExtent;
}

// The Gaussian of an occupied slot: the count, the world mean of the three coordinate sums in metres and, with kCov, the population
// covariance {xx, xy, xz, yy, yz, zz} in m^2 from the slot's nine moments.
struct Gaussian {
  uint32_t count;
  double mean[3], cov[6];
};

// The two parts of it, which align also applies to a source record: a coordinate's mean in metres from its fixed-point sum over n
// points, and the covariance from the nine sums S of the n points' 12-bit local coordinates, both on the grid of `voxel`.
__device__ __forceinline__ double sum_mean(long long sum, double n, double voxel) {
#pragma clang fp contract(off)
  return static_cast<double>(sum) / n / kScale * voxel;
}

__device__ __forceinline__ void sums_covariance(const double (&S)[kPlanes], double n, double voxel, double (&cov)[6]) {
#pragma clang fp contract(off)
  const double s = voxel / kMomSteps, s2 = s * s;
  const double m[3] = {S[0] / n, S[1] / n, S[2] / n};
  for (int a = 0, k = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b, ++k) cov[k] = (S[3 + k] / n - m[a] * m[b]) * s2;
}

template <bool kCov>
__device__ __forceinline__ Gaussian voxel_gaussian(const Table& t, const unsigned long long* __restrict__ moments, long long capacity,
                                                   double voxel, long long slot) {
  Gaussian g;
  g.count = t.counts[slot];
  const double n = static_cast<double>(g.count);
  for (int d = 0; d < 3; ++d) g.mean[d] = sum_mean(static_cast<long long>(t.sums[d * capacity + slot]), n, voxel);
  if constexpr (kCov) {
    double S[kPlanes];
    for (int k = 0; k < kPlanes; ++k) S[k] = static_cast<double>(static_cast<long long>(moments[moment_at(slot, k, capacity)]));
    sums_covariance(S, n, voxel, g.cov);
  }
  return g;
}

// What register and query weigh a residual with: M = (cov + sigma2 I)^-1, cofactors over the determinant, and Mr = M r.
__device__ __forceinline__ void voxel_precision(const double (&cov)[6], double sigma2, const double (&r)[3], double (&M)[3][3],
                                                double (&Mr)[3]) {
#pragma clang fp contract(off)
  const double a00 = cov[0] + sigma2, a01 = cov[1], a02 = cov[2], a11 = cov[3] + sigma2, a12 = cov[4], a22 = cov[5] + sigma2;
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  M[0][0] = c00 / det;
  M[0][1] = M[1][0] = c01 / det;
  M[0][2] = M[2][0] = c02 / det;
  M[1][1] = c11 / det;
  M[1][2] = M[2][1] = c12 / det;
  M[2][2] = c22 / det;
#pragma unroll
  for (int d = 0; d < 3; ++d) Mr[d] = (M[d][0] * r[0] + M[d][1] * r[1]) + M[d][2] * r[2];
}

// the number of offsets[1 .. n_scans] that are <= i: the scan of row i when offsets ascend (empty scans are passed over)
__device__ __forceinline__ long long scan_of(const int64_t* __restrict__ offsets, long long n_scans, long long i) {
  long long lo = 0, n = n_scans;
  while (n > 0) {
    const long long half = n >> 1;
    if (offsets[lo + half + 1] <= i) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

// The integrate kernels.  kMoments = false: `moments` is unused and every moments statement is compiled out; kObserved = false: the
// same for `obs` and `first_id` (the last arguments, so the plain kernels read theirs where they always did).  With kObserved the
// scan's position in the batch is its bit, so n_scans <= kMaxObsScans, and its id is first_id + that position.
template <bool kMoments, bool kObserved>
__global__ void __launch_bounds__(kBlock) integrate_kernel(Table t, unsigned long long* __restrict__ moments, long long capacity,
                                                           int channels, double voxel, const float* __restrict__ points, long long ld,
                                                           long long total, const int64_t* __restrict__ offsets,
                                                           const double* __restrict__ poses, long long n_scans, double lo2, double hi2,
                                                           Observations obs, int first_id) {
#pragma clang fp contract(off)
  __shared__ unsigned int tally[kStats];
  if (threadIdx.x < kStats) tally[threadIdx.x] = 0u;
  __syncthreads();
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  long long begin = offsets[0], end = offsets[n_scans];
  begin = begin < 0 ? 0 : begin;
  end = end > total ? total : end;  // (a bad offsets array reads nothing outside the batch)
  for (long long i = begin + static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < end; i += stride) {
    float v[kMaxC];
    double wd[3];
    long long q[kMaxC];
    [[maybe_unused]] int bit = 0;  // kObserved: the scan's position in the batch
    int verdict = gate_sensor(points + i * ld, channels, lo2, hi2, v);
    if (verdict == kPass) {
      const long long scan = scan_of(offsets, n_scans, i);
      if (scan >= n_scans) continue;  // (offsets that do not ascend)
      if constexpr (kObserved) bit = static_cast<int>(scan);
      verdict = gate_world(v, poses + scan * 16, voxel, wd, q);
    }
    if (verdict != kPass) {
      atomicAdd(&tally[verdict], 1u);
      continue;
    }
    int claimed;
    const long long slot = find_or_claim(t.keys, capacity, pack_key(q[0] >> kFrac, q[1] >> kFrac, q[2] >> kFrac), &claimed);
    if (slot < 0) {
      atomicAdd(&tally[kDropped], 1u);
      continue;
    }
    if (claimed) atomicAdd(&tally[kOccupied], 1u);
    atomicAdd(&tally[kIntegrated], 1u);
    atomicAdd(t.counts + slot, 1u);
    for (int c = 0; c < kMaxC; ++c)
      if (c < channels) atomicAdd(t.sums + c * capacity + slot, static_cast<unsigned long long>(q[c]));
    if constexpr (kMoments) {
      unsigned long long u[3];
      for (int d = 0; d < 3; ++d) u[d] = static_cast<unsigned long long>((q[d] - ((q[d] >> kFrac) << kFrac)) >> kMomShift);
      int k = 0;
      for (int d = 0; d < 3; ++d) atomicAdd(moments + moment_at(slot, k++, capacity), u[d]);
      for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) atomicAdd(moments + moment_at(slot, k++, capacity), u[a] * u[b]);
    }
    if constexpr (kObserved) {
      const unsigned long long seen = 1ull << bit;  // (bit < n_scans <= 64)
      if ((ld_agent(obs.mask + slot) & seen) == 0ull && (atomicOr(obs.mask + slot, seen) & seen) == 0ull) {
        const int id = first_id + bit;  // this thread is the voxel's first sighting of the scan
        atomicAdd(obs.record + observed_at(slot, kObsScans), 1);
        atomicMin(obs.record + observed_at(slot, kObsFirst), id);
        atomicMax(obs.record + observed_at(slot, kObsLast), id);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kStats && tally[threadIdx.x] != 0u)
    atomicAdd(t.counters + threadIdx.x, static_cast<unsigned long long>(tally[threadIdx.x]));
}

__global__ void __launch_bounds__(kBlock) moments_reset_kernel(unsigned long long* __restrict__ moments, long long words) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < words; i += stride) moments[i] = 0ull;
}

// The slot of `key` in a table that is not being written, or -1: the probe ends at the key, at an empty slot or after one cycle.
__device__ __forceinline__ long long find(const unsigned long long* __restrict__ keys, long long capacity, unsigned long long key) {
  const unsigned long long mask = static_cast<unsigned long long>(capacity) - 1ull;
  unsigned long long slot = mix(key) & mask;
  for (long long probe = 0; probe < capacity; ++probe) {
    const unsigned long long k = keys[slot];
    if (k == key) return static_cast<long long>(slot);
    if (k == kEmpty) return -1;
    slot = (slot + 1ull) & mask;
  }
  return -1;
}

// After rehash_kernel moved the table `a` into `b`: what a second block holds for every occupied slot of `a` into the slot its key has
// in `b` (the new block reset before; the keys are distinct, so plain stores).  copy(i, slot): the block's payload, below.
template <class Copy>
__global__ void __launch_bounds__(kBlock) block_rehash_kernel(Table a, long long cap_a, Table b, long long cap_b, Copy copy) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < cap_a; i += stride) {
    const unsigned long long key = a.keys[i];
    if (key == kEmpty) continue;
    const long long slot = find(b.keys, cap_b, key);
    if (slot < 0) continue;  // (a key that the map's rehash did not move: the voxels that rdm_voxel_map_prune left behind)
    copy(i, slot);
  }
}

struct MomentsCopy {  // the nine sums
  const unsigned long long* __restrict__ from;
  unsigned long long* __restrict__ to;
  long long cap_a, cap_b;
  __device__ void operator()(long long i, long long slot) const {
    unsigned long long v[kPlanes];  // (nine loads in flight, then nine stores: `restrict` on a member does not license that)
    for (int k = 0; k < kPlanes; ++k) v[k] = from[moment_at(i, k, cap_a)];
    for (int k = 0; k < kPlanes; ++k) to[moment_at(slot, k, cap_b)] = v[k];
  }
};

// The sweep before an integrate call (records = false: the masks alone) and the reset: no scan seen, first = kMaxScanId, last = -1.
__global__ void __launch_bounds__(kBlock) observations_reset_kernel(Observations o, long long capacity, bool records) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < capacity; i += stride) {
    o.mask[i] = 0ull;
    if (records) {
      o.record[observed_at(i, kObsScans)] = 0;
      o.record[observed_at(i, kObsFirst)] = static_cast<int>(kMaxScanId);
      o.record[observed_at(i, kObsLast)] = -1;
    }
  }
}

struct RecordsCopy {  // block_rehash_kernel's payload of the observations: the record; the mask is scratch and stays behind
  const int* __restrict__ from;
  int* __restrict__ to;
  __device__ void operator()(long long i, long long slot) const {
    for (int k = 0; k < kObsFields; ++k) to[observed_at(slot, k)] = from[observed_at(i, k)];
  }
};

// Every occupied slot of `a` into `b` (reset before): the keys are distinct, so a slot is claimed once and filled with plain stores.
// kPrune (rdm_voxel_map_prune): only the slots with at least min_points points seen in at least min_scans scans (`oa`: the records of
// `a`), and `occupied` and `integrated` are counted over those; the other arguments are unused without it.
template <bool kPrune>
__global__ void __launch_bounds__(kBlock) rehash_kernel(Table a, long long cap_a, Table b, long long cap_b, int channels, Observations oa,
                                                        unsigned int min_points, int min_scans) {
  __shared__ unsigned long long kept[2];  // voxels, points
  if constexpr (kPrune) {
    if (threadIdx.x < 2) kept[threadIdx.x] = 0ull;
    __syncthreads();
  }
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (first < kStats && !(kPrune && first <= kIntegrated)) b.counters[first] = a.counters[first];
  for (long long i = first; i < cap_a; i += stride) {
    const unsigned long long key = a.keys[i];
    if (key == kEmpty) continue;
    if (kPrune && (a.counts[i] < min_points || oa.record[observed_at(i, kObsScans)] < min_scans)) continue;
    int claimed;
    const long long slot = find_or_claim(b.keys, cap_b, key, &claimed);
    if (slot < 0 || !claimed) continue;  // (cap_b >= cap_a and distinct keys: not reached)
    b.counts[slot] = a.counts[i];
    for (int c = 0; c < channels; ++c) b.sums[c * cap_b + slot] = a.sums[c * cap_a + i];
    if constexpr (kPrune) {
      atomicAdd(&kept[0], 1ull);
      atomicAdd(&kept[1], static_cast<unsigned long long>(a.counts[i]));
    }
  }
  if constexpr (kPrune) {  // (reset_kernel left both counters of `b` at zero)
    __syncthreads();
    if (threadIdx.x < 2 && kept[threadIdx.x] != 0ull) atomicAdd(b.counters + threadIdx.x, kept[threadIdx.x]);
  }
}
static_assert(kOccupied == 0 && kIntegrated == 1, "rehash_kernel<true> counts these two");

__global__ void __launch_bounds__(kBlock) select_kernel(Table t, long long capacity, unsigned int min_points,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ slots,
                                                        unsigned long long* __restrict__ n_rows) {
  __shared__ unsigned int picked;
  if (threadIdx.x == 0) picked = 0u;
  __syncthreads();
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < capacity; i += stride) {
    const unsigned long long key = t.keys[i];
    const bool take = key != kEmpty && t.counts[i] >= min_points;
    keys[i] = take ? key : kEmpty;
    slots[i] = static_cast<int>(i);
    if (take) atomicAdd(&picked, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && picked != 0u) atomicAdd(n_rows, static_cast<unsigned long long>(picked));
}

__global__ void __launch_bounds__(kBlock) emit_kernel(Table t, long long capacity, int channels, double voxel,
                                                      const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                      const unsigned long long* __restrict__ n_sel, long long max_rows,
                                                      float* __restrict__ points, int32_t* __restrict__ counts,
                                                      int32_t* __restrict__ cells, int64_t* __restrict__ n_rows) {
#pragma clang fp contract(off)
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const long long m = static_cast<long long>(*n_sel);
  if (first == 0) *n_rows = m;
  const long long rows = m < max_rows ? m : max_rows;
  for (long long r = first; r < rows; r += stride) {
    const long long slot = slots[r];
    const Gaussian g = voxel_gaussian<false>(t, nullptr, capacity, voxel, slot);
    counts[r] = static_cast<int32_t>(g.count);
    for (int d = 0; d < 3; ++d) {
      cells[3 * r + d] = static_cast<int32_t>(key_cell(keys[r], d));
      points[r * channels + d] = static_cast<float>(g.mean[d]);
    }
    for (int c = 3; c < channels; ++c)  // an attribute's mean is not scaled by the voxel
      points[r * channels + c] =
          static_cast<float>(static_cast<double>(static_cast<long long>(t.sums[c * capacity + slot])) / static_cast<double>(g.count) / kScale);
  }
}

// Eigenvalues (ascending) and the unit eigenvector of the smallest one of the symmetric matrix {xx, xy, xz, yy, yz, zz}: cyclic
// Jacobi, kSweeps sweeps over (0,1), (0,2), (1,2) with Rutishauser's update.  A rotation whose off-diagonal entry is already zero
// is passed over, so a diagonal matrix (a single point: all zeros) comes back as it is.  No trigonometric closed form: that loses
// the small eigenvalue of a planar voxel to cancellation.
__device__ __forceinline__ void jacobi3(const double* __restrict__ cov, double* __restrict__ eig, double* __restrict__ normal) {
  double a[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // (theta = +-inf: t = 0)
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
      a[p][p] -= t * apq;
      a[q][q] += t * apq;
      a[p][q] = a[q][p] = 0.0;
      const double arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
      a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = vkp - s * (vkq + tau * vkp);
        v[k][q] = vkq + s * (vkp - tau * vkq);
      }
    }
  }
  // ascending, ties in index order
  int i0 = 0, i1 = 1, i2 = 2;
  if (a[i1][i1] < a[i0][i0]) { const int x = i0; i0 = i1; i1 = x; }
  if (a[i2][i2] < a[i1][i1]) { const int x = i1; i1 = i2; i2 = x; }
  if (a[i1][i1] < a[i0][i0]) { const int x = i0; i0 = i1; i1 = x; }
  eig[0] = a[i0][i0];
  eig[1] = a[i1][i1];
  eig[2] = a[i2][i2];
  double n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) n[k] = i0 == 0 ? v[k][0] : (i0 == 1 ? v[k][1] : v[k][2]);
  const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  int big = 0;  // the component of largest magnitude is positive; on a tie the lowest axis decides
  if (fabs(n[1]) > fabs(n[big])) big = 1;
  if (fabs(n[2]) > fabs(n[big])) big = 2;
  const double sign = (big == 0 ? n[0] : (big == 1 ? n[1] : n[2])) < 0.0 ? -1.0 : 1.0;
  for (int k = 0; k < 3; ++k) normal[k] = sign * n[k] / len;
}

__global__ void __launch_bounds__(kBlock) emit_moments_kernel(Table t, const unsigned long long* __restrict__ moments, long long capacity,
                                                              double voxel, const int* __restrict__ slots,
                                                              const unsigned long long* __restrict__ n_sel, long long max_rows,
                                                              int64_t* __restrict__ sums, double* __restrict__ cov,
                                                              double* __restrict__ eigenvalues, double* __restrict__ normals,
                                                              int64_t* __restrict__ n_rows) {
#pragma clang fp contract(off)
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const long long m = static_cast<long long>(*n_sel);
  if (first == 0) *n_rows = m;
  const long long rows = m < max_rows ? m : max_rows;
  for (long long r = first; r < rows; r += stride) {
    const long long slot = slots[r];
    if (sums != nullptr)
      for (int k = 0; k < kPlanes; ++k) sums[r * kPlanes + k] = static_cast<long long>(moments[moment_at(slot, k, capacity)]);
    const Gaussian g = voxel_gaussian<true>(t, moments, capacity, voxel, slot);
    double eig[3], normal[3];
    jacobi3(g.cov, eig, normal);
    for (int k = 0; k < 6; ++k) cov[r * 6 + k] = g.cov[k];
    for (int k = 0; k < 3; ++k) {
      eigenvalues[r * 3 + k] = eig[k];
      normals[r * 3 + k] = normal[k];
    }
  }
}

__global__ void __launch_bounds__(kBlock) emit_observations_kernel(Observations o, const int* __restrict__ slots,
                                                                   const unsigned long long* __restrict__ n_sel, long long max_rows,
                                                                   int32_t* __restrict__ scans, int32_t* __restrict__ first_seen,
                                                                   int32_t* __restrict__ last_seen, int64_t* __restrict__ n_rows) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const long long m = static_cast<long long>(*n_sel);
  if (first == 0) *n_rows = m;
  const long long rows = m < max_rows ? m : max_rows;
  for (long long r = first; r < rows; r += stride) {
    const long long slot = slots[r];
    scans[r] = o.record[observed_at(slot, kObsScans)];
    first_seen[r] = o.record[observed_at(slot, kObsFirst)];
    last_seen[r] = o.record[observed_at(slot, kObsLast)];
  }
}

// The raw state of the selected rows (rdm_voxel_map_export): what integrate added, as it stands in the slot.  Any output may be null;
// `moments` / `records` are null exactly when their output is.
__global__ void __launch_bounds__(kBlock) emit_state_kernel(Table t, const unsigned long long* __restrict__ moments,
                                                            const int* __restrict__ records, long long capacity, int channels,
                                                            const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                            const unsigned long long* __restrict__ n_sel, long long max_rows,
                                                            unsigned long long* __restrict__ out_keys, uint32_t* __restrict__ counts,
                                                            int64_t* __restrict__ sums, int64_t* __restrict__ moment_sums,
                                                            int32_t* __restrict__ seen, int64_t* __restrict__ n_rows) {
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const long long m = static_cast<long long>(*n_sel);
  if (first == 0) *n_rows = m;
  const long long rows = m < max_rows ? m : max_rows;
  for (long long r = first; r < rows; r += stride) {
    const long long slot = slots[r];
    if (out_keys != nullptr) out_keys[r] = keys[r];
    if (counts != nullptr) counts[r] = t.counts[slot];
    if (sums != nullptr)
      for (int c = 0; c < channels; ++c) sums[r * channels + c] = static_cast<long long>(t.sums[c * capacity + slot]);
    if (moment_sums != nullptr)
      for (int k = 0; k < kPlanes; ++k) moment_sums[r * kPlanes + k] = static_cast<long long>(moments[moment_at(slot, k, capacity)]);
    if (seen != nullptr)
      for (int k = 0; k < kObsFields; ++k) seen[r * kObsFields + k] = records[observed_at(slot, k)];
  }
}

// rdm_voxel_map_import: one thread per record of the layout that emit_state_kernel writes.  A record is a voxel's worth of points that
// integrate has summed already, so it goes where a point goes -- find_or_claim, then integer atomic adds (two records of a batch may
// hold the same key) -- with `count` in the place of 1.  `moments` / `obs.record` are null when the map lacks the block; moment_sums /
// seen are read only where the block is there.  skipped: the four skip counters of the map the records come from, added once.
enum { kImpOccupied = 0, kImpIntegrated, kImpDropped, kImpRejected, kImpTallies };
struct Skipped {
  unsigned long long v[4];  // skipped_nonfinite, skipped_range, out_of_extent, dropped_full
};
static_assert(kNonfinite == 2 && kDropped == 5, "Skipped follows the counters from kNonfinite on");

__global__ void __launch_bounds__(kBlock) import_kernel(Table t, unsigned long long* __restrict__ moments, Observations obs,
                                                        long long capacity, int channels, const unsigned long long* __restrict__ keys,
                                                        const uint32_t* __restrict__ counts, const int64_t* __restrict__ sums,
                                                        const int64_t* __restrict__ moment_sums, const int32_t* __restrict__ seen,
                                                        long long n_records, int id_offset, Skipped skipped,
                                                        unsigned long long* __restrict__ n_rejected) {
  __shared__ unsigned long long tally[kImpTallies];
  if (threadIdx.x < kImpTallies) tally[threadIdx.x] = 0ull;
  __syncthreads();
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (first < 4 && skipped.v[first] != 0ull) atomicAdd(t.counters + kNonfinite + first, skipped.v[first]);
  for (long long i = first; i < n_records; i += stride) {
    const unsigned long long key = keys[i];
    const uint32_t count = counts[i];
    bool valid = (key >> 63) == 0ull && count != 0u;
    int rec[kObsFields] = {0, 0, 0};
    if (seen != nullptr) {
      for (int k = 0; k < kObsFields; ++k) rec[k] = seen[i * kObsFields + k];
      const long long scans = rec[kObsScans], lo = rec[kObsFirst], hi = rec[kObsLast];
      valid = valid && scans >= 1 && lo >= 0 && lo <= hi && scans <= hi - lo + 1 && hi <= kMaxScanId - 1 - id_offset;
    }
    if (!valid) {
      atomicAdd(&tally[kImpRejected], 1ull);
      continue;
    }
    int claimed;
    const long long slot = find_or_claim(t.keys, capacity, key, &claimed);
    if (slot < 0) {
      atomicAdd(&tally[kImpDropped], static_cast<unsigned long long>(count));
      continue;
    }
    if (claimed) atomicAdd(&tally[kImpOccupied], 1ull);
    atomicAdd(&tally[kImpIntegrated], static_cast<unsigned long long>(count));
    atomicAdd(t.counts + slot, count);  // (wraps at 2^32, as a count does)
    for (int c = 0; c < channels; ++c) atomicAdd(t.sums + c * capacity + slot, static_cast<unsigned long long>(sums[i * channels + c]));
    if (moments != nullptr)
      for (int k = 0; k < kPlanes; ++k)
        atomicAdd(moments + moment_at(slot, k, capacity), static_cast<unsigned long long>(moment_sums[i * kPlanes + k]));
    if (obs.record != nullptr) {
      atomicAdd(obs.record + observed_at(slot, kObsScans), rec[kObsScans]);
      atomicMin(obs.record + observed_at(slot, kObsFirst), rec[kObsFirst] + id_offset);
      atomicMax(obs.record + observed_at(slot, kObsLast), rec[kObsLast] + id_offset);
    }
  }
  __syncthreads();
  if (threadIdx.x < kImpTallies && tally[threadIdx.x] != 0ull) {
    const int k = threadIdx.x;
    atomicAdd(k == kImpRejected ? n_rejected : t.counters + (k == kImpDropped ? kDropped : k), tally[k]);
  }
}

unsigned blocks_for(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return static_cast<unsigned>(b < 1 ? 1 : (b > static_cast<int64_t>(kMaxBlocks) ? kMaxBlocks : b));
}

struct ExtractWork {
  unsigned long long *keys_in, *keys, *n_sel;
  int *slots_in, *slots;
  void* sort_tmp;
  size_t sort_bytes;
};

bool carve_extract(Arena& ar, int64_t capacity, ExtractWork& w) {
  const size_t s = static_cast<size_t>(capacity);
  w.n_sel = ar.take<unsigned long long>(1);
  w.keys_in = ar.take<unsigned long long>(s);
  w.keys = ar.take<unsigned long long>(s);
  w.slots_in = ar.take<int>(s);
  w.slots = ar.take<int>(s);
  w.sort_bytes = sort_temp_bytes(capacity);
  w.sort_tmp = ar.take<char>(w.sort_bytes > 0 ? w.sort_bytes : 1);
  return ar.ok;
}

// the table of a caller's block, or the error code after set_error
int open_table(const char* what, void* map, size_t map_bytes, int64_t capacity, int channels, Table& t) {
  RDM_REQUIRE(shape_ok(capacity, channels),
              "%s: capacity must be a power of two in [64, 2^30] and channels 3 ... %d, got %lld and %d", what, kMaxC,
              static_cast<long long>(capacity), channels);
  RDM_REQUIRE(map != nullptr, "%s: null map", what);
  Arena ar(map, map_bytes);
  if (!carve(ar, capacity, channels, t)) {
    set_error("%s: the map block is too small (%zu < %zu bytes)", what, map_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  return RDM_OK;
}

// the moments block of a caller, or the error code after set_error (`too_small`: the code for a block that is too small)
int open_moments(const char* what, const void* moments, size_t moments_bytes, int64_t capacity, unsigned long long*& m,
                 int too_small = RDM_ERR_WORKSPACE) {
  RDM_REQUIRE(moments != nullptr, "%s: null moments block", what);
  Arena ar(const_cast<void*>(moments), moments_bytes);
  m = ar.take<unsigned long long>(static_cast<size_t>(capacity) * kPlanes);
  if (!ar.ok) {
    set_error("%s: the moments block is too small (%zu < %zu bytes)", what, moments_bytes, ar.off);
    return too_small;
  }
  return RDM_OK;
}

// the observations block of a caller, or the error code after set_error
int open_observations(const char* what, const void* observations, size_t observations_bytes, int64_t capacity, Observations& o) {
  RDM_REQUIRE(observations != nullptr, "%s: null observations block", what);
  Arena ar(const_cast<void*>(observations), observations_bytes);
  if (!carve_observations(ar, capacity, o)) {
    set_error("%s: the observations block is too small (%zu < %zu bytes)", what, observations_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  return RDM_OK;
}

// A caller's map with the blocks beside it.  A block's pointer and size stand for how the entry point takes it: kAbsent (not looked
// at), kOptional (opened when the pointer is not null) or kRequired (a null pointer is an error).
struct Blocks {
  Table t;
  unsigned long long* m = nullptr;
  Observations o{nullptr, nullptr};
};
enum Want { kAbsent, kOptional, kRequired };
struct BlockArg {
  Want want;
  const void* p;
  size_t bytes;
};
constexpr BlockArg kNoBlock{kAbsent, nullptr, 0};

// the blocks of a caller, or the error code after set_error (moments_too_small: open_moments' too_small)
int open_blocks(const char* what, const void* map, size_t map_bytes, int64_t capacity, int channels, BlockArg moments,
                BlockArg observations, Blocks& b, int moments_too_small = RDM_ERR_WORKSPACE) {
  if (const int rc = open_table(what, const_cast<void*>(map), map_bytes, capacity, channels, b.t)) return rc;
  if (moments.want == kRequired || (moments.want == kOptional && moments.p != nullptr))
    if (const int rc = open_moments(what, moments.p, moments.bytes, capacity, b.m, moments_too_small)) return rc;
  if (observations.want == kRequired || (observations.want == kOptional && observations.p != nullptr))
    if (const int rc = open_observations(what, observations.p, observations.bytes, capacity, b.o)) return rc;
  return RDM_OK;
}

// The two sides of a rehash or a prune: the old blocks `a` and the new ones `b`, which must be other blocks of at least the old
// capacity.  At most one of moments and observations moves with the map.
int open_rehash(const char* what, const void* old_map, size_t old_bytes, int64_t old_capacity, BlockArg old_m, BlockArg old_o,
                const void* new_map, size_t new_bytes, int64_t new_capacity, BlockArg new_m, BlockArg new_o, int channels, Blocks& a,
                Blocks& b) {
  const std::string name(what);
  if (const int rc = open_blocks((name + " (old)").c_str(), old_map, old_bytes, old_capacity, channels, old_m, old_o, a)) return rc;
  if (const int rc = open_blocks((name + " (new)").c_str(), new_map, new_bytes, new_capacity, channels, new_m, new_o, b)) return rc;
  const bool mom = new_m.want != kAbsent, obs = new_o.want != kAbsent;
  const bool other = new_capacity >= old_capacity && new_map != old_map && (!mom || new_m.p != old_m.p) && (!obs || new_o.p != old_o.p);
  if (!mom && !obs)
    RDM_REQUIRE(other, "%s: the new map must be another block of at least the old capacity", what);
  else
    RDM_REQUIRE(other, "%s: the new map and %s must be other blocks of at least the old capacity", what, mom ? "moments" : "observations");
  return RDM_OK;
}

// ---- scan-to-map registration (include/rdmnet_hip.h, "voxel map registration"; tests/voxel_register_restatement.py) --------------
//
// An iteration is two launches.  accumulate_kernel: kRegGroups workgroups per scan; row j of a scan goes to thread
// j mod (kRegGroups kBlock) of the scan's threads, whatever else the batch holds, so a scan's sums are the same wherever it stands.
// A thread keeps the upper triangle of H (21), g (6), the cost and two counts, block_sum adds them in a fixed order and one slab row
// per workgroup is written.  register_finalize_kernel: one workgroup per scan adds the scan's slab rows in index order, thread 0
// factors H, moves the pose, tests convergence and writes the outputs.  No float atomics; the table is only read.
//
// Robust weights (rdm_voxel_map_register_robust, robust_scale mu > 0; tests/voxel_register_robust_restatement.py) are a second
// instantiation, kRobust, of accumulate_pairs and of both kernels: per pair d2 = r^T M r, s = mu / (mu + d2), l = s s; every term of
// H and g is multiplied by l before it is added, the cost takes s d2, and a 31st sum, l itself, goes to slot 30 of the slab row and
// from there to weight_sums.  The plain instantiation has none of this in it -- weighted<false> is the identity, no multiply is
// compiled -- and it never writes or reads slot 30.

constexpr int kRegGroups = 64;   // workgroups per scan
constexpr int kRegSums = 30;     // H upper triangle, g, cost, then n_corr and the gated points (integers, exact in a double)
constexpr int kRegSumsRobust = kRegSums + 1;  // and the sum of the weights
constexpr int kRegRow = 32;      // doubles per slab row
static_assert(kRegSumsRobust <= kRegRow, "a slab row holds the sums of either form");
constexpr int kRegChunk = 8;     // evaluations enqueued between two reads of `running`
constexpr int64_t kMaxRegScans = int64_t(1) << 20;  // kRegGroups workgroups each in one grid

struct RegState {
  double X[16];  // the pose of the next evaluation
  int updates;   // applied so far
  int last;      // the next evaluation is the one after convergence
  int done;
  int pad;
};

struct RegWork {
  RegState* st;  // [n_scans]
  double* slab;  // [n_scans][kRegGroups][kRegRow]
  int* running;  // scans that are not done
};

bool carve_register(Arena& ar, int64_t n_scans, RegWork& w) {
  const size_t n = static_cast<size_t>(n_scans > 0 ? n_scans : 1);
  w.running = ar.take<int>(1);
  w.st = ar.take<RegState>(n);
  w.slab = ar.take<double>(n * kRegGroups * kRegRow);
  return ar.ok;
}

__global__ void __launch_bounds__(kBlock) register_init_kernel(const double* __restrict__ poses, long long n_scans, RegWork w) {
  const long long s = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (s == 0) *w.running = static_cast<int>(n_scans);
  if (s >= n_scans) return;
  RegState& st = w.st[s];
  for (int k = 0; k < 16; ++k) st.X[k] = poses[s * 16 + k];
  st.updates = 0;
  st.last = 0;
  st.done = 0;
  st.pad = 0;
}

// The visit of register, align and query: pair(o, slot) for o = 0 ... visits - 1 -- the cell itself, then its -x, +x, -y, +y, -z, +z
// neighbour -- wherever that cell lies in the extent and its slot holds at least min_points points.  (A loop around the body and no
// function that returns a slot or -1: behind such a return the compiler reads the slot's count a second time.)
template <class Pair>
__device__ __forceinline__ void for_each_neighbor(const Table& t, long long capacity, const long long (&cell)[3], int visits,
                                                  unsigned int min_points, Pair&& pair) {
  for (int o = 0; o < visits; ++o) {
    long long c[3] = {cell[0], cell[1], cell[2]};
    if (o > 0) c[(o - 1) >> 1] += (o & 1) ? -1 : 1;
    if (c[0] < -kHalf || c[0] >= kHalf || c[1] < -kHalf || c[1] >= kHalf || c[2] < -kHalf || c[2] >= kHalf) continue;
    const long long slot = find(t.keys, capacity, pack_key(c[0], c[1], c[2]));
    if (slot < 0 || t.counts[slot] < min_points) continue;
    pair(o, slot);
  }
}

// A pair's term under its weight l: the term itself where the pairs are not weighted (no multiply is compiled).
template <bool kRobust>
__device__ __forceinline__ double weighted(double l, double x) {
#pragma clang fp contract(off)
  if constexpr (kRobust)
    return l * x;
  else
    return x;
}

// What the accumulate kernel does with one world point wd of the cell `cell` at the pose X: the visit and, per pair, H's upper triangle,
// g and the cost into acc.  kExtra: `extra`, six covariance entries, is added to the voxel's own before the inverse (align: the
// source's R Sigma_b R^T); else it is not looked at (register).  kRobust: every pair is weighted by l = (mu / (mu + d2))^2, d2 its
// cost term, and acc[kRegSums] takes the sum of l; else mu is not looked at and acc has no such slot.  -> the number of pairs.
template <bool kExtra, bool kRobust>
__device__ __forceinline__ int accumulate_pairs(const Table& t, const unsigned long long* __restrict__ moments, long long capacity,
                                                double voxel, const double (&wd)[3], const long long (&cell)[3], const double (&X)[12],
                                                const double* extra, double sigma2, unsigned int min_points, int neighbors,
                                                double (&acc)[kRobust ? kRegSumsRobust : kRegSums], double mu) {
#pragma clang fp contract(off)
  int n_corr = 0;
  const double q0 = wd[0] - X[3], q1 = wd[1] - X[7], q2 = wd[2] - X[11];
  for_each_neighbor(t, capacity, cell, neighbors, min_points, [&](int, long long slot) {
    Gaussian G = voxel_gaussian<true>(t, moments, capacity, voxel, slot);
    if constexpr (kExtra) {
#pragma unroll
      for (int k = 0; k < 6; ++k) G.cov[k] = G.cov[k] + extra[k];
    }
    const double r[3] = {wd[0] - G.mean[0], wd[1] - G.mean[1], wd[2] - G.mean[2]};
    double M[3][3], Mr[3];
    voxel_precision(G.cov, sigma2, r, M, Mr);
    // B = [q]x M = (J's rotation block)^T M; H = [[-B [q]x, B], [B^T, M]], g = (q x Mr, Mr)
    double B[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      B[0][j] = q1 * M[2][j] - q2 * M[1][j];
      B[1][j] = q2 * M[0][j] - q0 * M[2][j];
      B[2][j] = q0 * M[1][j] - q1 * M[0][j];
    }
    double Hrr[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      Hrr[a][0] = B[a][2] * q1 - B[a][1] * q2;
      Hrr[a][1] = B[a][0] * q2 - B[a][2] * q0;
      Hrr[a][2] = B[a][1] * q0 - B[a][0] * q1;
    }
    const double d2 = (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
    [[maybe_unused]] double s = 1.0, l = 1.0;
    if constexpr (kRobust) {
      s = mu / (mu + d2);
      l = s * s;
      acc[kRegSums] += l;
    }
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = a; b < 3; ++b) acc[k++] += weighted<kRobust>(l, Hrr[a][b]);
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[k++] += weighted<kRobust>(l, B[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = a; b < 3; ++b) acc[k++] += weighted<kRobust>(l, M[a][b]);
    acc[21] += weighted<kRobust>(l, q1 * Mr[2] - q2 * Mr[1]);
    acc[22] += weighted<kRobust>(l, q2 * Mr[0] - q0 * Mr[2]);
    acc[23] += weighted<kRobust>(l, q0 * Mr[1] - q1 * Mr[0]);
    acc[24] += weighted<kRobust>(l, Mr[0]);
    acc[25] += weighted<kRobust>(l, Mr[1]);
    acc[26] += weighted<kRobust>(l, Mr[2]);
    acc[27] += weighted<kRobust>(s, d2);
    ++n_corr;
  });
  return n_corr;
}

// The rows that the accumulate kernel sums over.  row(i, X, voxel, wd, cell, extra) -> whether row i takes part at the pose X on the
// target's grid of `voxel`: then wd is its world point and `cell` that point's cell; with kExtra, `extra` is what accumulate_pairs
// adds to a voxel's covariance.
//
// register: a scan's point behind the point gate.
struct PointRow {
  static constexpr bool kExtra = false;
  const float* __restrict__ points;
  long long ld;
  int channels;
  double lo2, hi2;
  __device__ __forceinline__ bool operator()(long long i, const double (&X)[12], double voxel, double (&wd)[3], long long (&cell)[3],
                                             double*) const {
    float v[kMaxC];
    long long q[kMaxC];
    if (gate_sensor(points + i * ld, channels, lo2, hi2, v) != kPass || gate_world(v, X, voxel, wd, q) != kPass) return false;
    for (int d = 0; d < 3; ++d) cell[d] = q[d] >> kFrac;
    return true;
  }
};

// align (include/rdmnet_hip.h, "voxel map alignment"; tests/voxel_align_restatement.py): a voxel record of the source map in the place
// of a point.  The record's mean is the point, under world_fixed on the target's grid, and its covariance Sigma_b, turned by the pose,
// is the extra: C = (R Sigma_b) R^T, upper triangle.
struct RecordRow {
  static constexpr bool kExtra = true;
  const uint32_t* __restrict__ counts;
  const long long* __restrict__ sums;
  long long sums_ld;
  const long long* __restrict__ moment_sums;
  double source_voxel;
  unsigned int source_min_points;
  __device__ __forceinline__ bool operator()(long long i, const double (&X)[12], double voxel, double (&wd)[3], long long (&cell)[3],
                                             double* C) const {
#pragma clang fp contract(off)
    const uint32_t count = counts[i];
    if (count < source_min_points) return false;
    const double n = static_cast<double>(count);
    double mu[3];
    for (int d = 0; d < 3; ++d) mu[d] = sum_mean(sums[i * sums_ld + d], n, source_voxel);
    long long q[3];
    if (!world_fixed(X, mu[0], mu[1], mu[2], voxel, wd, q)) return false;
    for (int d = 0; d < 3; ++d) cell[d] = q[d] >> kFrac;
    double S[kPlanes], cb[6];
    for (int k = 0; k < kPlanes; ++k) S[k] = static_cast<double>(moment_sums[i * kPlanes + k]);
    sums_covariance(S, n, source_voxel, cb);
    const double Sb[3][3] = {{cb[0], cb[1], cb[2]}, {cb[1], cb[3], cb[4]}, {cb[2], cb[4], cb[5]}};
    double P[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) P[a][b] = (X[4 * a] * Sb[0][b] + X[4 * a + 1] * Sb[1][b]) + X[4 * a + 2] * Sb[2][b];
    for (int a = 0, k = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b, ++k) C[k] = (P[a][0] * X[4 * b] + P[a][1] * X[4 * b + 1]) + P[a][2] * X[4 * b + 2];
    return true;
  }
};

// The accumulate launch of register (PointRow) and align (RecordRow): kRegGroups workgroups per scan or source, as described above.
template <bool kRobust, class Row>
__global__ void __launch_bounds__(kBlock) accumulate_kernel(Table t, const unsigned long long* __restrict__ moments, long long capacity,
                                                            double voxel, Row row, long long total, const int64_t* __restrict__ offsets,
                                                            double sigma2, unsigned int min_points, int neighbors, RegWork w, double mu) {
  constexpr int kSums = kRobust ? kRegSumsRobust : kRegSums;
  const long long scan = blockIdx.x / kRegGroups;
  const int group = blockIdx.x % kRegGroups;
  const RegState& st = w.st[scan];
  if (st.done) return;
  double X[12];
  for (int k = 0; k < 12; ++k) X[k] = st.X[k];
  long long begin = offsets[scan], end = offsets[scan + 1];
  begin = begin < 0 ? 0 : begin;
  end = end > total ? total : end;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  int n_corr = 0, n_pass = 0;
  for (long long i = begin + group * kBlock + threadIdx.x; i < end; i += static_cast<long long>(kRegGroups) * kBlock) {
    double wd[3];
    long long cell[3];
    [[maybe_unused]] double extra[6];
    if (!row(i, X, voxel, wd, cell, extra)) continue;
    ++n_pass;
    n_corr += accumulate_pairs<Row::kExtra, kRobust>(t, moments, capacity, voxel, wd, cell, X, extra, sigma2, min_points, neighbors, acc, mu);
  }
  acc[28] = static_cast<double>(n_corr);
  acc[29] = static_cast<double>(n_pass);
  const double sum = block_sum<kSums, kBlock>(acc, threadIdx.x);
  if (threadIdx.x < kSums) w.slab[(scan * kRegGroups + group) * kRegRow + threadIdx.x] = sum;
}

// Exp(omega) by Rodrigues' formula: I + a [omega]x + b [omega]x^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 (their series below 1e-4).
__device__ __forceinline__ void rodrigues(const double* __restrict__ om, double (&E)[3][3]) {
  const double th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2];
  const double th = sqrt(th2);
  double a, b;
  if (th < 1e-4) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
  } else {
    a = sin(th) / th;
    b = (1.0 - cos(th)) / th2;
  }
  const double K[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      E[i][j] = ((i == j ? 1.0 : 0.0) + a * K[i][j]) + b * kk;
    }
}

// kRobust: the slab rows hold kRegSumsRobust sums and weight_sums takes the last; else they hold kRegSums, slot 30 is not read and
// weight_sums takes n_corr, the sum of weights that are all one.  weight_sums may be null.
template <bool kRobust>
__global__ void __launch_bounds__(kBlock) register_finalize_kernel(RegWork w, int max_iteration, double rot_eps, double trans_eps,
                                                                   double* __restrict__ transforms, double* __restrict__ hessians,
                                                                   double* __restrict__ gradients, double* __restrict__ costs,
                                                                   int64_t* __restrict__ stats, double* __restrict__ weight_sums) {
#pragma clang fp contract(off)
  constexpr int kSums = kRobust ? kRegSumsRobust : kRegSums;
  const long long scan = blockIdx.x;
  RegState& st = w.st[scan];
  if (st.done) return;
  __shared__ double tot[kSums];
  if (threadIdx.x < kSums) {
    const double* rows = w.slab + scan * kRegGroups * kRegRow + threadIdx.x;
    double sum = rows[0];
    for (int g = 1; g < kRegGroups; ++g) sum += rows[g * kRegRow];
    tot[threadIdx.x] = sum;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double H[6][6], g[6];
  int k = 0;
  for (int a = 0; a < 3; ++a) {
    for (int b = a; b < 3; ++b) H[a][b] = H[b][a] = tot[k++];
    for (int b = 0; b < 3; ++b) H[a][3 + b] = H[3 + b][a] = tot[k++];
  }
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) H[3 + a][3 + b] = H[3 + b][3 + a] = tot[k++];
  for (int a = 0; a < 6; ++a) g[a] = tot[21 + a];
  const long long n_corr = static_cast<long long>(tot[28]), n_pass = static_cast<long long>(tot[29]);
  // the outputs describe the pose just evaluated
  for (int q = 0; q < 16; ++q) transforms[scan * 16 + q] = st.X[q];
  for (int a = 0; a < 6; ++a) {
    for (int b = 0; b < 6; ++b) hessians[scan * 36 + a * 6 + b] = H[a][b];
    gradients[scan * 6 + a] = g[a];
  }
  costs[scan] = tot[27];
  if (weight_sums != nullptr) weight_sums[scan] = kRobust ? tot[kSums - 1] : static_cast<double>(n_corr);
  int status = -1;  // running
  if (st.last) {
    status = 1;
  } else if (st.updates >= max_iteration) {
    status = 0;
  } else {
    // H = L L^T without pivoting, L y = -g, L^T delta = y
    double L[6][6], y[6], delta[6];
    bool good = n_corr > 0;
    for (int j = 0; j < 6 && good; ++j) {
      double d = H[j][j];
      for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
      if (!(d > 0.0) || !isfinite(d)) {
        good = false;
        break;
      }
      L[j][j] = sqrt(d);
      for (int i = j + 1; i < 6; ++i) {
        double v = H[i][j];
        for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
        L[i][j] = v / L[j][j];
      }
    }
    if (!good) {
      status = 2;
    } else {
      for (int i = 0; i < 6; ++i) {
        double v = -g[i];
        for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
        y[i] = v / L[i][i];
      }
      for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 6; ++q) v -= L[q][i] * delta[q];
        delta[i] = v / L[i][i];
      }
      double E[3][3], R[3][3];
      rodrigues(delta, E);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = (E[i][0] * st.X[j] + E[i][1] * st.X[4 + j]) + E[i][2] * st.X[8 + j];
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) st.X[4 * i + j] = R[i][j];
        st.X[4 * i + 3] = st.X[4 * i + 3] + delta[3 + i];
      }
      st.updates += 1;
      const double rot = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
      const double trans = sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
      if (rot < rot_eps && trans < trans_eps) st.last = 1;
    }
  }
  stats[scan * 4 + 0] = st.updates;
  stats[scan * 4 + 1] = n_corr;
  stats[scan * 4 + 2] = n_pass;
  stats[scan * 4 + 3] = status;
  if (status >= 0) {
    st.done = 1;
    atomicSub(w.running, 1);
  }
}

// ---- per-point queries (include/rdmnet_hip.h, "voxel map queries"; tests/voxel_query_restatement.py) ----------------------------
//
// One launch, one thread per row, a read-only gather: the gates and the lookup of register, but what the lookup finds is kept per
// row and not summed.  A workgroup takes a contiguous run of 256-row chunks, so the rows of one scan that it meets are tallied in LDS
// (wave ballots, one LDS add per wave and field) and reach the scan's row of `tallies` as one integer atomic per field when the run
// leaves the scan.  kDist = false is the labels-only form of neighbors = 1: no sums, no moments and no float64 beyond the gates.

constexpr unsigned kQueryBlocks = 2048;  // 8 workgroups on each of 256 CUs; longer batches go to longer runs of chunks
constexpr int kTallies = RDM_VOXEL_QUERY_TALLIES;
constexpr int kNoLabel = kTallies;  // of a thread without a row
static_assert(kTallies == 8 && RDM_VOXEL_POINT_STATIC == 6, "seven labels and the pairs in a row of tallies");
static_assert(RDM_VOXEL_POINT_NONFINITE == 0 && kRange - kNonfinite == RDM_VOXEL_POINT_RANGE &&
                  kExtent - kNonfinite == RDM_VOXEL_POINT_EXTENT,
              "a gate's verdict is its label + kNonfinite");

struct QueryOut {  // any of them null: not computed, not written
  uint8_t* labels;
  int8_t* best;
  int32_t* counts;
  int32_t* seen;
  double* d2;
  double* d2_sum;
  uint8_t* pairs;
  unsigned long long* tallies;
};

template <bool kDist, bool kCov>
__global__ void __launch_bounds__(kBlock) query_kernel(Table t, const unsigned long long* __restrict__ moments,
                                                       const int* __restrict__ records, long long capacity, int channels, double voxel,
                                                       const float* __restrict__ points, long long ld, long long total,
                                                       const int64_t* __restrict__ offsets, const double* __restrict__ poses,
                                                       long long n_scans, double lo2, double hi2, double sigma2, unsigned int min_points,
                                                       int neighbors, int min_scans, double max_d2, long long chunks, QueryOut out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long tally[kTallies];
  if (threadIdx.x < kTallies) tally[threadIdx.x] = 0ull;
  long long tallied = -1;  // the scan that `tally` counts
  // every thread of the workgroup calls it with the same `next`
  auto turn_to = [&](long long next) {
    __syncthreads();
    if (threadIdx.x < kTallies && tally[threadIdx.x] != 0ull) {
      atomicAdd(out.tallies + tallied * kTallies + threadIdx.x, tally[threadIdx.x]);  // (nothing was counted while tallied = -1)
      tally[threadIdx.x] = 0ull;
    }
    __syncthreads();
    tallied = next;
  };
  long long begin = offsets[0], end = offsets[n_scans];
  begin = begin < 0 ? 0 : begin;
  end = end > total ? total : end;  // (a bad offsets array reads and writes nothing outside the batch)
  const int visits = kDist ? neighbors : 1;
  for (long long c = 0; c < chunks; ++c) {
    const long long row0 = begin + (static_cast<long long>(blockIdx.x) * chunks + c) * kBlock;
    if (row0 >= end) break;
    const long long i = row0 + threadIdx.x;
    long long scan = -1;
    int label = kNoLabel, pairs = 0;
    if (i < end && (scan = scan_of(offsets, n_scans, i)) < n_scans) {
      float v[kMaxC];
      double wd[3];
      long long q[kMaxC];
      int verdict = gate_sensor(points + i * ld, channels, lo2, hi2, v);
      if (verdict == kPass) verdict = gate_world(v, poses + scan * 16, voxel, wd, q);
      int best = -1;
      long long best_slot = -1;
      uint32_t best_count = 0u;
      [[maybe_unused]] double best_d2 = INFINITY, sum = 0.0;
      int seen[kObsFields] = {0, static_cast<int>(kMaxScanId), -1};
      if (verdict != kPass) {
        label = verdict - kNonfinite;
      } else {
        const long long cell[3] = {q[0] >> kFrac, q[1] >> kFrac, q[2] >> kFrac};
        for_each_neighbor(t, capacity, cell, visits, min_points, [&](int o, long long slot) {
          const uint32_t count = t.counts[slot];
          ++pairs;
          if constexpr (kDist) {
            Gaussian G = voxel_gaussian<kCov>(t, moments, capacity, voxel, slot);
            if constexpr (!kCov)
              for (int k = 0; k < 6; ++k) G.cov[k] = 0.0;
            const double r[3] = {wd[0] - G.mean[0], wd[1] - G.mean[1], wd[2] - G.mean[2]};
            double M[3][3], Mr[3];
            voxel_precision(G.cov, sigma2, r, M, Mr);
            const double d2 = (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];  // (accumulate_pairs' d2)
            sum += d2;
            if (best >= 0 && !(d2 < best_d2)) return;  // ties go to the smallest o
            best_d2 = d2;
          }
          best = o;
          best_slot = slot;
          best_count = count;
        });
        if (best >= 0 && records != nullptr)
          for (int k = 0; k < kObsFields; ++k) seen[k] = records[observed_at(best_slot, k)];
        if (best < 0)
          label = RDM_VOXEL_POINT_UNMAPPED;
        else if (records != nullptr && seen[kObsScans] < min_scans)
          label = RDM_VOXEL_POINT_TRANSIENT;
        else if (kDist && best_d2 > max_d2)
          label = RDM_VOXEL_POINT_OFF_SURFACE;
        else
          label = RDM_VOXEL_POINT_STATIC;
      }
      if (out.labels != nullptr) out.labels[i] = static_cast<uint8_t>(label);
      if (out.best != nullptr) out.best[i] = static_cast<int8_t>(best);
      if (out.counts != nullptr) out.counts[i] = static_cast<int32_t>(best_count);
      if (out.seen != nullptr)
        for (int k = 0; k < kObsFields; ++k) out.seen[i * kObsFields + k] = seen[k];
      if constexpr (kDist) {
        if (out.d2 != nullptr) out.d2[i] = best_d2;
        if (out.d2_sum != nullptr) out.d2_sum[i] = sum;
      }
      if (out.pairs != nullptr) out.pairs[i] = static_cast<uint8_t>(pairs);
    }
    if (out.tallies == nullptr) continue;
    // the scans of this chunk's rows, one after the other (one, as a rule); an empty scan has no row to count
    const long long last_row = (row0 + kBlock < end ? row0 + kBlock : end) - 1;
    long long last = scan_of(offsets, n_scans, last_row);
    last = last < n_scans ? last : n_scans - 1;
    for (long long s = scan_of(offsets, n_scans, row0); s <= last; ++s) {
      if (offsets[s + 1] <= offsets[s]) continue;
      if (s != tallied) turn_to(s);
      const bool mine = scan == s && label != kNoLabel;
      unsigned long long add[kTallies];
      for (int k = 0; k < kTallies - 1; ++k) add[k] = __popcll(__ballot(mine && label == k));
      add[kTallies - 1] = 0ull;  // pairs <= 7: three bits
      for (int b = 0; b < 3; ++b) add[kTallies - 1] += static_cast<unsigned long long>(__popcll(__ballot(mine && ((pairs >> b) & 1)))) << b;
      if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kTallies; ++k)
          if (add[k] != 0ull) atomicAdd(&tally[k], add[k]);
    }
  }
  if (out.tallies != nullptr && tallied >= 0) turn_to(-1);
}

// ---- what the entry points share -----------------------------------------------------------------------------------------------

// The batch arguments of integrate and register, or the error code after set_error.  max_scans: kMaxRegScans or no limit; empty_runs:
// the entry point launches for n_scans > 0 even when the batch has no rows, so it reads offsets and poses then too.
int check_batch(const char* what, double voxel, int channels, const float* points, int64_t ld, int64_t total, const int64_t* offsets,
                const double* poses, int64_t n_scans, int64_t max_scans, bool empty_runs, double min_range, double max_range) {
  RDM_REQUIRE(voxel > 0.0 && std::isfinite(voxel), "%s: voxel must be positive and finite", what);
  RDM_REQUIRE(n_scans >= 0 && n_scans <= max_scans && total >= 0 && ld >= channels, "%s: bad sizes (ld must be >= channels%s)", what,
              max_scans == kMaxRegScans ? ", n_scans <= 2^20" : "");
  RDM_REQUIRE(min_range >= 0.0 && max_range >= min_range, "%s: need 0 <= min_range <= max_range", what);
  const bool rows = n_scans > 0 && total > 0, scans = rows || (empty_runs && n_scans > 0);
  RDM_REQUIRE((!rows || points) && (!scans || (offsets && poses)), "%s: null argument", what);
  return RDM_OK;
}

// rdm_voxel_map_integrate (want_moments = false: `moments` is not looked at), rdm_voxel_map_integrate_moments and, with observed,
// rdm_voxel_map_integrate_observed: the batch's scans have the ids first_id, first_id + 1, ...
int integrate(const char* what, void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, const float* points, int64_t ld,
              int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans, double min_range, double max_range,
              bool want_moments, void* moments, size_t moments_bytes, bool observed, void* observations, size_t observations_bytes,
              int64_t first_id, void* stream) {
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {want_moments ? kRequired : kAbsent, moments, moments_bytes},
                                 {observed ? kRequired : kAbsent, observations, observations_bytes}, b))
    return rc;
  RDM_REQUIRE(!observed || (n_scans <= kMaxObsScans && first_id >= 0 && first_id <= kMaxScanId - (n_scans > 0 ? n_scans : 0)),
              "%s: a call takes at most %d scans and ids in [0, 2^31 - 1), got %lld scans from id %lld", what, kMaxObsScans,
              static_cast<long long>(n_scans), static_cast<long long>(first_id));
  if (const int rc = check_batch(what, voxel, channels, points, ld, total, offsets, poses, n_scans, INT64_MAX, false, min_range, max_range))
    return rc;
  if (n_scans == 0 || total == 0) return RDM_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (observed)  // the masks of the call before
    hipLaunchKernelGGL(observations_reset_kernel, dim3(blocks_for(capacity)), dim3(kBlock), 0, s, b.o, static_cast<long long>(capacity), false);
  auto kernel = observed ? (want_moments ? integrate_kernel<true, true> : integrate_kernel<false, true>)
                         : (want_moments ? integrate_kernel<true, false> : integrate_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks_for(total)), dim3(kBlock), 0, s, b.t, b.m, capacity, channels, voxel, points, ld, total, offsets,
                     poses, n_scans, min_range * min_range, max_range * max_range, b.o, static_cast<int>(first_id));
  return launch_status(what);
}

unsigned int least_points(int64_t min_points) {  // (counts are uint32)
  return min_points > 0xffffffffll ? 0xffffffffu : static_cast<unsigned int>(min_points);
}

// The lookup options of register, align and query, or RDM_ERR_ARG after set_error.  rest_ok / rest: the entry point's own bounds and
// their text ("min_points >= 1, ...").
int check_options(const char* what, double sigma, int neighbors, bool rest_ok, const char* rest) {
  RDM_REQUIRE(sigma > 0.0 && std::isfinite(sigma), "%s: sigma must be positive and finite (got %g)", what, sigma);
  RDM_REQUIRE(neighbors == 1 || neighbors == 7, "%s: neighbors must be 1 or 7 (got %d)", what, neighbors);
  RDM_REQUIRE(rest_ok, "%s: need %s", what, rest);
  return RDM_OK;
}

// The Gauss-Newton iteration of register and align from the initial `poses` of n scans or sources: the workspace, the init launch,
// then chunks of kRegChunk evaluations -- accumulate(w), the caller's accumulate launch on `s`, and the finalize launch -- with one
// 4-byte read-back of `running` between two chunks.  robust: the slab rows hold the sum of the weights, which goes to weight_sums.
template <class Accumulate>
int gauss_newton(const char* what, const double* poses, int64_t n, int max_iteration, double rot_eps, double trans_eps, bool robust,
                 double* transforms, double* hessians, double* gradients, double* costs, double* weight_sums, int64_t* stats, void* ws,
                 size_t ws_bytes, hipStream_t s, Accumulate accumulate) {
  Arena ar(ws, ws_bytes);
  RegWork w;
  if (!carve_register(ar, n, w)) {
    set_error("%s: workspace too small (%zu < %zu bytes)", what, ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  if (n == 0) return RDM_OK;
  RDM_REQUIRE(transforms && hessians && gradients && costs && stats, "%s: null output", what);
  hipLaunchKernelGGL(register_init_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, s, poses, static_cast<long long>(n), w);
  int running = 1;
  for (int k = 0; k <= max_iteration && running > 0;) {
    const int end = max_iteration - k < kRegChunk ? max_iteration + 1 : k + kRegChunk;
    for (; k < end; ++k) {
      accumulate(w);
      hipLaunchKernelGGL(robust ? register_finalize_kernel<true> : register_finalize_kernel<false>, dim3(static_cast<unsigned>(n)),
                         dim3(kBlock), 0, s, w, max_iteration, rot_eps, trans_eps, transforms, hessians, gradients, costs, stats, weight_sums);
    }
    if (const int rc = launch_status(what)) return rc;
    RDM_HIP_CHECK(hipMemcpyAsync(&running, w.running, sizeof(int), hipMemcpyDeviceToHost, s));  // one 4-byte read-back per chunk
    RDM_HIP_CHECK(hipStreamSynchronize(s));
  }
  return RDM_OK;
}

// What both extracts do before they emit: the argument checks (outputs_ok: the entry point's own outputs are there), then the slots
// with at least min_points points selected and sorted by key -> w.keys, w.slots and their number *w.n_sel on the device.
int select_sorted(const char* what, const Table& t, int64_t capacity, double voxel, int64_t min_points, int64_t max_rows,
                  const int64_t* n_rows, bool outputs_ok, void* ws, size_t ws_bytes, hipStream_t s, ExtractWork& w) {
  RDM_REQUIRE(voxel > 0.0 && std::isfinite(voxel), "%s: voxel must be positive and finite", what);
  RDM_REQUIRE(min_points >= 0 && max_rows >= 0 && n_rows != nullptr, "%s: bad min_points, max_rows or null n_rows", what);
  RDM_REQUIRE(outputs_ok, "%s: null output", what);
  Arena ar(ws, ws_bytes);
  if (!carve_extract(ar, capacity, w)) {
    set_error("%s: workspace too small (%zu < %zu bytes)", what, ws_bytes, ar.off);
    return RDM_ERR_WORKSPACE;
  }
  fill_words<unsigned long long>(w.n_sel, 1, 0ull, s);
  hipLaunchKernelGGL(select_kernel, dim3(blocks_for(capacity)), dim3(kBlock), 0, s, t, static_cast<long long>(capacity),
                     least_points(min_points), w.keys_in, w.slots_in, w.n_sel);
  size_t bytes = w.sort_bytes;
  RDM_HIP_CHECK(rocprim::radix_sort_pairs(w.sort_tmp, bytes, w.keys_in, w.keys, w.slots_in, w.slots, static_cast<unsigned>(capacity), 0u,
                                          64u, s));
  return RDM_OK;
}

}  // namespace
}  // namespace rdm

extern "C" size_t rdm_voxel_map_bytes(int64_t capacity, int channels) {
  using namespace rdm;
  if (!shape_ok(capacity, channels)) return 0;
  Arena ar(nullptr, 0);
  Table t;
  carve(ar, capacity, channels, t);
  return ar.off;
}

extern "C" int rdm_voxel_map_reset(void* map, size_t map_bytes, int64_t capacity, int channels, void* stream) {
  using namespace rdm;
  Blocks b;
  if (const int rc = open_blocks("rdm_voxel_map_reset", map, map_bytes, capacity, channels, kNoBlock, kNoBlock, b)) return rc;
  hipLaunchKernelGGL(reset_kernel, dim3(blocks_for(capacity)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), b.t,
                     static_cast<long long>(capacity), channels);
  return launch_status("rdm_voxel_map_reset");
}

extern "C" int rdm_voxel_map_integrate(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel, const float* points,
                                       int64_t ld, int64_t total, const int64_t* offsets, const double* poses, int64_t n_scans,
                                       double min_range, double max_range, void* stream) {
  return rdm::integrate("rdm_voxel_map_integrate", map, map_bytes, capacity, channels, voxel, points, ld, total, offsets, poses, n_scans,
                        min_range, max_range, false, nullptr, 0, false, nullptr, 0, 0, stream);
}

extern "C" int rdm_voxel_map_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, void* new_map, size_t new_bytes,
                                    int64_t new_capacity, int channels, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_rehash";
  Blocks a, b;
  if (const int rc = open_rehash(what, old_map, old_bytes, old_capacity, kNoBlock, kNoBlock, new_map, new_bytes, new_capacity, kNoBlock, kNoBlock,
                                 channels, a, b))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reset_kernel, dim3(blocks_for(new_capacity)), dim3(kBlock), 0, s, b.t, static_cast<long long>(new_capacity), channels);
  hipLaunchKernelGGL(rehash_kernel<false>, dim3(blocks_for(old_capacity)), dim3(kBlock), 0, s, a.t, static_cast<long long>(old_capacity),
                     b.t, static_cast<long long>(new_capacity), channels, Observations{nullptr, nullptr}, 0u, 0);
  return launch_status(what);
}

extern "C" int rdm_voxel_map_stats(const void* map, size_t map_bytes, int64_t capacity, int channels, uint64_t* stats, void* stream) {
  using namespace rdm;
  Blocks b;
  if (const int rc = open_blocks("rdm_voxel_map_stats", map, map_bytes, capacity, channels, kNoBlock, kNoBlock, b)) return rc;
  RDM_REQUIRE(stats != nullptr, "rdm_voxel_map_stats: null stats");
  hipStream_t s = static_cast<hipStream_t>(stream);
  RDM_HIP_CHECK(hipMemcpyAsync(stats, b.t.counters, kStats * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  RDM_HIP_CHECK(hipStreamSynchronize(s));
  return RDM_OK;
}

extern "C" size_t rdm_voxel_map_extract_workspace_bytes(int64_t capacity) {
  using namespace rdm;
  if (!shape_ok(capacity, 3)) return 0;
  Arena ar(nullptr, 0);
  ExtractWork w;
  carve_extract(ar, capacity, w);
  return ar.off;
}

extern "C" int rdm_voxel_map_extract(const void* map, size_t map_bytes, int64_t capacity, int channels, double voxel,
                                     int64_t min_points, float* points, int32_t* counts, int32_t* cells, int64_t max_rows,
                                     int64_t* n_rows, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  Blocks b;
  if (const int rc = open_blocks("rdm_voxel_map_extract", map, map_bytes, capacity, channels, kNoBlock, kNoBlock, b)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ExtractWork w;
  if (const int rc = select_sorted("rdm_voxel_map_extract", b.t, capacity, voxel, min_points, max_rows, n_rows,
                                   max_rows == 0 || (points && counts && cells), ws, ws_bytes, s, w))
    return rc;
  hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(max_rows)), dim3(kBlock), 0, s, b.t, static_cast<long long>(capacity), channels, voxel,
                     w.keys, w.slots, w.n_sel, static_cast<long long>(max_rows), points, counts, cells, n_rows);
  return launch_status("rdm_voxel_map_extract");
}

// ---- voxel moments ------------------------------------------------------------------------------------------------------------

extern "C" size_t rdm_voxel_moments_bytes(int64_t capacity) {
  using namespace rdm;
  if (!shape_ok(capacity, 3)) return 0;
  Arena ar(nullptr, 0);
  ar.take<unsigned long long>(static_cast<size_t>(capacity) * kPlanes);
  return ar.off;
}

extern "C" int rdm_voxel_moments_reset(void* moments, size_t moments_bytes, int64_t capacity, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(shape_ok(capacity, 3), "rdm_voxel_moments_reset: capacity must be a power of two in [64, 2^30], got %lld",
              static_cast<long long>(capacity));
  unsigned long long* m;
  if (const int rc = open_moments("rdm_voxel_moments_reset", moments, moments_bytes, capacity, m)) return rc;
  hipLaunchKernelGGL(moments_reset_kernel, dim3(blocks_for(capacity * kPlanes)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), m,
                     static_cast<long long>(capacity) * kPlanes);
  return launch_status("rdm_voxel_moments_reset");
}

extern "C" int rdm_voxel_map_integrate_moments(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel,
                                               const float* points, int64_t ld, int64_t total, const int64_t* offsets,
                                               const double* poses, int64_t n_scans, double min_range, double max_range, void* moments,
                                               size_t moments_bytes, void* stream) {
  return rdm::integrate("rdm_voxel_map_integrate_moments", map, map_bytes, capacity, channels, voxel, points, ld, total, offsets, poses,
                        n_scans, min_range, max_range, true, moments, moments_bytes, false, nullptr, 0, 0, stream);
}

extern "C" int rdm_voxel_moments_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_moments,
                                        size_t old_moments_bytes, const void* new_map, size_t new_bytes, int64_t new_capacity,
                                        void* new_moments, size_t new_moments_bytes, int channels, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_moments_rehash";
  Blocks a, b;
  if (const int rc = open_rehash(what, old_map, old_bytes, old_capacity, {kRequired, old_moments, old_moments_bytes}, kNoBlock, new_map, new_bytes,
                                 new_capacity, {kRequired, new_moments, new_moments_bytes}, kNoBlock, channels, a, b))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(moments_reset_kernel, dim3(blocks_for(new_capacity * kPlanes)), dim3(kBlock), 0, s, b.m,
                     static_cast<long long>(new_capacity) * kPlanes);
  hipLaunchKernelGGL(block_rehash_kernel<MomentsCopy>, dim3(blocks_for(old_capacity)), dim3(kBlock), 0, s, a.t,
                     static_cast<long long>(old_capacity), b.t, static_cast<long long>(new_capacity),
                     MomentsCopy{a.m, b.m, static_cast<long long>(old_capacity), static_cast<long long>(new_capacity)});
  return launch_status(what);
}

extern "C" int rdm_voxel_map_extract_moments(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                             size_t moments_bytes, double voxel, int64_t min_points, int64_t* sums, double* cov,
                                             double* eigenvalues, double* normals, int64_t max_rows, int64_t* n_rows, void* ws,
                                             size_t ws_bytes, void* stream) {
  using namespace rdm;
  Blocks b;
  if (const int rc = open_blocks("rdm_voxel_map_extract_moments", map, map_bytes, capacity, channels, {kRequired, moments, moments_bytes},
                                 kNoBlock, b))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ExtractWork w;
  if (const int rc = select_sorted("rdm_voxel_map_extract_moments", b.t, capacity, voxel, min_points, max_rows, n_rows,
                                   max_rows == 0 || (cov && eigenvalues && normals), ws, ws_bytes, s, w))
    return rc;
  hipLaunchKernelGGL(emit_moments_kernel, dim3(blocks_for(max_rows)), dim3(kBlock), 0, s, b.t, b.m, static_cast<long long>(capacity), voxel,
                     w.slots, w.n_sel, static_cast<long long>(max_rows), sums, cov, eigenvalues, normals, n_rows);
  return launch_status("rdm_voxel_map_extract_moments");
}

// ---- voxel observations -------------------------------------------------------------------------------------------------------

extern "C" size_t rdm_voxel_observations_bytes(int64_t capacity) {
  using namespace rdm;
  if (!shape_ok(capacity, 3)) return 0;
  Arena ar(nullptr, 0);
  Observations o;
  carve_observations(ar, capacity, o);
  return ar.off;
}

extern "C" int rdm_voxel_observations_reset(void* observations, size_t observations_bytes, int64_t capacity, void* stream) {
  using namespace rdm;
  RDM_REQUIRE(shape_ok(capacity, 3), "rdm_voxel_observations_reset: capacity must be a power of two in [64, 2^30], got %lld",
              static_cast<long long>(capacity));
  Observations o;
  if (const int rc = open_observations("rdm_voxel_observations_reset", observations, observations_bytes, capacity, o)) return rc;
  hipLaunchKernelGGL(observations_reset_kernel, dim3(blocks_for(capacity)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), o,
                     static_cast<long long>(capacity), true);
  return launch_status("rdm_voxel_observations_reset");
}

extern "C" int rdm_voxel_map_integrate_observed(void* map, size_t map_bytes, int64_t capacity, int channels, double voxel,
                                                const float* points, int64_t ld, int64_t total, const int64_t* offsets,
                                                const double* poses, int64_t n_scans, double min_range, double max_range, void* moments,
                                                size_t moments_bytes, void* observations, size_t observations_bytes, int64_t first_id,
                                                void* stream) {
  return rdm::integrate("rdm_voxel_map_integrate_observed", map, map_bytes, capacity, channels, voxel, points, ld, total, offsets, poses,
                        n_scans, min_range, max_range, moments != nullptr, moments, moments_bytes, true, observations, observations_bytes,
                        first_id, stream);
}

extern "C" int rdm_voxel_observations_rehash(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_observations,
                                             size_t old_observations_bytes, const void* new_map, size_t new_bytes, int64_t new_capacity,
                                             void* new_observations, size_t new_observations_bytes, int channels, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_observations_rehash";
  Blocks a, b;
  if (const int rc = open_rehash(what, old_map, old_bytes, old_capacity, kNoBlock, {kRequired, old_observations, old_observations_bytes}, new_map,
                                 new_bytes, new_capacity, kNoBlock, {kRequired, new_observations, new_observations_bytes}, channels, a, b))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(observations_reset_kernel, dim3(blocks_for(new_capacity)), dim3(kBlock), 0, s, b.o, static_cast<long long>(new_capacity), true);
  hipLaunchKernelGGL(block_rehash_kernel<RecordsCopy>, dim3(blocks_for(old_capacity)), dim3(kBlock), 0, s, a.t,
                     static_cast<long long>(old_capacity), b.t, static_cast<long long>(new_capacity), RecordsCopy{a.o.record, b.o.record});
  return launch_status(what);
}

extern "C" int rdm_voxel_map_extract_observations(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* observations,
                                                  size_t observations_bytes, double voxel, int64_t min_points, int32_t* scans,
                                                  int32_t* first, int32_t* last, int64_t max_rows, int64_t* n_rows, void* ws,
                                                  size_t ws_bytes, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_extract_observations";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, kNoBlock, {kRequired, observations, observations_bytes}, b)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  ExtractWork w;
  if (const int rc = select_sorted(what, b.t, capacity, voxel, min_points, max_rows, n_rows, max_rows == 0 || (scans && first && last), ws,
                                   ws_bytes, s, w))
    return rc;
  hipLaunchKernelGGL(emit_observations_kernel, dim3(blocks_for(max_rows)), dim3(kBlock), 0, s, b.o, w.slots, w.n_sel,
                     static_cast<long long>(max_rows), scans, first, last, n_rows);
  return launch_status(what);
}

extern "C" int rdm_voxel_map_prune(const void* old_map, size_t old_bytes, int64_t old_capacity, const void* old_observations,
                                   size_t old_observations_bytes, void* new_map, size_t new_bytes, int64_t new_capacity, int channels,
                                   int64_t min_points, int64_t min_scans, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_prune";
  Blocks a, b;
  if (const int rc = open_rehash(what, old_map, old_bytes, old_capacity, kNoBlock, kNoBlock, new_map, new_bytes, new_capacity, kNoBlock, kNoBlock,
                                 channels, a, b))
    return rc;
  if (const int rc = open_observations(what, old_observations, old_observations_bytes, old_capacity, a.o)) return rc;  // (no " (old)")
  RDM_REQUIRE(min_points >= 0 && min_scans >= 0, "%s: min_points and min_scans must be >= 0", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reset_kernel, dim3(blocks_for(new_capacity)), dim3(kBlock), 0, s, b.t, static_cast<long long>(new_capacity), channels);
  hipLaunchKernelGGL(rehash_kernel<true>, dim3(blocks_for(old_capacity)), dim3(kBlock), 0, s, a.t, static_cast<long long>(old_capacity), b.t,
                     static_cast<long long>(new_capacity), channels, a.o, least_points(min_points),
                     static_cast<int>(min_scans > kMaxScanId ? kMaxScanId : min_scans));
  return launch_status(what);
}

// ---- voxel map state ----------------------------------------------------------------------------------------------------------

extern "C" int rdm_voxel_map_export(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                    size_t moments_bytes, const void* observations, size_t observations_bytes, int64_t min_points,
                                    uint64_t* keys, uint32_t* counts, int64_t* sums, int64_t* moment_sums, int32_t* seen, int64_t max_rows,
                                    int64_t* n_rows, void* ws, size_t ws_bytes, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_export";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {kOptional, moments, moments_bytes},
                                 {kOptional, observations, observations_bytes}, b))
    return rc;
  RDM_REQUIRE((b.m != nullptr || moment_sums == nullptr) && (b.o.record != nullptr || seen == nullptr),
              "%s: moment_sums needs a moments block and seen an observations block", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ExtractWork w;
  if (const int rc = select_sorted(what, b.t, capacity, 1.0, min_points, max_rows, n_rows, true, ws, ws_bytes, s, w)) return rc;
  hipLaunchKernelGGL(emit_state_kernel, dim3(blocks_for(max_rows)), dim3(kBlock), 0, s, b.t, moment_sums != nullptr ? b.m : nullptr,
                     seen != nullptr ? b.o.record : nullptr, static_cast<long long>(capacity), channels, w.keys, w.slots, w.n_sel,
                     static_cast<long long>(max_rows), reinterpret_cast<unsigned long long*>(keys), counts, sums, moment_sums, seen, n_rows);
  return launch_status(what);
}

extern "C" int rdm_voxel_map_import(void* map, size_t map_bytes, int64_t capacity, int channels, void* moments, size_t moments_bytes,
                                    void* observations, size_t observations_bytes, const uint64_t* keys, const uint32_t* counts,
                                    const int64_t* sums, const int64_t* moment_sums, const int32_t* seen, int64_t n_records,
                                    int64_t id_offset, const uint64_t* skipped_host, int64_t* n_rejected, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_import";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {kOptional, moments, moments_bytes},
                                 {kOptional, observations, observations_bytes}, b))
    return rc;
  RDM_REQUIRE(n_records >= 0 && n_rejected != nullptr, "%s: n_records must be >= 0 and n_rejected not null", what);
  RDM_REQUIRE(id_offset >= 0 && id_offset <= kMaxScanId, "%s: id_offset must be in [0, 2^31 - 1], got %lld", what,
              static_cast<long long>(id_offset));
  RDM_REQUIRE(n_records == 0 || (keys && counts && sums), "%s: null keys, counts or sums", what);
  RDM_REQUIRE((b.m != nullptr) == (moment_sums != nullptr) || (n_records == 0 && moment_sums == nullptr),
              "%s: moment_sums is required if and only if the map has a moments block", what);
  RDM_REQUIRE((b.o.record != nullptr) == (seen != nullptr) || (n_records == 0 && seen == nullptr),
              "%s: seen is required if and only if the map has an observations block", what);
  Skipped skipped{{0ull, 0ull, 0ull, 0ull}};
  if (skipped_host != nullptr)
    for (int k = 0; k < 4; ++k) skipped.v[k] = skipped_host[k];
  hipStream_t s = static_cast<hipStream_t>(stream);
  fill_words<unsigned long long>(reinterpret_cast<unsigned long long*>(n_rejected), 1, 0ull, s);
  hipLaunchKernelGGL(import_kernel, dim3(blocks_for(n_records)), dim3(kBlock), 0, s, b.t, b.m, b.o, static_cast<long long>(capacity), channels,
                     reinterpret_cast<const unsigned long long*>(keys), counts, sums, moment_sums, seen, static_cast<long long>(n_records),
                     static_cast<int>(id_offset), skipped, reinterpret_cast<unsigned long long*>(n_rejected));
  return launch_status(what);
}

// ---- voxel map registration ---------------------------------------------------------------------------------------------------

extern "C" size_t rdm_voxel_map_register_workspace_bytes(int64_t n_scans) {
  using namespace rdm;
  if (n_scans < 0 || n_scans > kMaxRegScans) return 0;
  Arena ar(nullptr, 0);
  RegWork w;
  carve_register(ar, n_scans, w);
  return ar.off;
}

extern "C" int rdm_voxel_map_register(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                      size_t moments_bytes, double voxel, const float* points, int64_t ld, int64_t total,
                                      const int64_t* offsets, const double* poses, int64_t n_scans, double min_range, double max_range,
                                      double sigma, int64_t min_points, int neighbors, int max_iteration, double rot_eps,
                                      double trans_eps, double* transforms, double* hessians, double* gradients, double* costs,
                                      int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
  return rdm_voxel_map_register_robust(map, map_bytes, capacity, channels, moments, moments_bytes, voxel, points, ld, total, offsets, poses,
                                       n_scans, min_range, max_range, sigma, min_points, neighbors, max_iteration, rot_eps, trans_eps, 0.0,
                                       transforms, hessians, gradients, costs, nullptr, stats, ws, ws_bytes, stream);
}

// (the messages keep the name rdm_voxel_map_register: it is this function with robust_scale = 0)
extern "C" int rdm_voxel_map_register_robust(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                             size_t moments_bytes, double voxel, const float* points, int64_t ld, int64_t total,
                                             const int64_t* offsets, const double* poses, int64_t n_scans, double min_range,
                                             double max_range, double sigma, int64_t min_points, int neighbors, int max_iteration,
                                             double rot_eps, double trans_eps, double robust_scale, double* transforms, double* hessians,
                                             double* gradients, double* costs, double* weight_sums, int64_t* stats, void* ws,
                                             size_t ws_bytes, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_register";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {kRequired, moments, moments_bytes}, kNoBlock, b, RDM_ERR_ARG))
    return rc;
  if (const int rc = check_batch(what, voxel, channels, points, ld, total, offsets, poses, n_scans, kMaxRegScans, true, min_range, max_range))
    return rc;
  if (const int rc = check_options(what, sigma, neighbors, min_points >= 1 && max_iteration >= 0 && rot_eps >= 0.0 && trans_eps >= 0.0,
                                   "min_points >= 1, max_iteration >= 0, rot_eps >= 0 and trans_eps >= 0"))
    return rc;
  RDM_REQUIRE(robust_scale >= 0.0 && std::isfinite(robust_scale),
              "rdm_voxel_map_register_robust: robust_scale must be finite and >= 0 (0: no weights; got %g)", robust_scale);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool robust = robust_scale > 0.0;
  const PointRow row{points, static_cast<long long>(ld), channels, min_range * min_range, max_range * max_range};
  auto kernel = robust ? accumulate_kernel<true, PointRow> : accumulate_kernel<false, PointRow>;
  return gauss_newton(what, poses, n_scans, max_iteration, rot_eps, trans_eps, robust, transforms, hessians, gradients, costs, weight_sums,
                      stats, ws, ws_bytes, s, [&](const RegWork& w) {
                        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(n_scans * kRegGroups)), dim3(kBlock), 0, s, b.t, b.m,
                                           static_cast<long long>(capacity), voxel, row, static_cast<long long>(total), offsets,
                                           sigma * sigma, least_points(min_points), neighbors, w, robust_scale);
                      });
}

// ---- voxel map alignment ------------------------------------------------------------------------------------------------------

extern "C" size_t rdm_voxel_map_align_workspace_bytes(int64_t n_sets) { return rdm_voxel_map_register_workspace_bytes(n_sets); }

extern "C" int rdm_voxel_map_align(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                   size_t moments_bytes, double voxel, const uint32_t* counts, const int64_t* sums, int64_t sums_ld,
                                   const int64_t* moment_sums, double source_voxel, int64_t total, const int64_t* offsets,
                                   const double* poses, int64_t n_sets, double sigma, int64_t min_points, int64_t source_min_points,
                                   int neighbors, int max_iteration, double rot_eps, double trans_eps, double* transforms,
                                   double* hessians, double* gradients, double* costs, int64_t* stats, void* ws, size_t ws_bytes,
                                   void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_align";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {kRequired, moments, moments_bytes}, kNoBlock, b, RDM_ERR_ARG))
    return rc;
  RDM_REQUIRE(voxel > 0.0 && std::isfinite(voxel), "%s: voxel must be positive and finite", what);
  RDM_REQUIRE(source_voxel > 0.0 && std::isfinite(source_voxel), "%s: source_voxel must be positive and finite", what);
  RDM_REQUIRE(n_sets >= 0 && n_sets <= kMaxRegScans && total >= 0, "%s: bad sizes (need total >= 0 and 0 <= n_sets <= 2^20)", what);
  RDM_REQUIRE(sums_ld >= 3, "%s: sums_ld must be >= 3 (got %lld)", what, static_cast<long long>(sums_ld));
  if (n_sets > 0 && total > 0) {
    RDM_REQUIRE(counts != nullptr, "%s: null counts", what);
    RDM_REQUIRE(sums != nullptr, "%s: null sums", what);
    RDM_REQUIRE(moment_sums != nullptr, "%s: null moment_sums", what);
  }
  RDM_REQUIRE(n_sets == 0 || (offsets && poses), "%s: null offsets or poses", what);
  if (const int rc = check_options(what, sigma, neighbors,
                                   min_points >= 1 && source_min_points >= 1 && max_iteration >= 0 && rot_eps >= 0.0 && trans_eps >= 0.0,
                                   "min_points >= 1, source_min_points >= 1, max_iteration >= 0, rot_eps >= 0 and trans_eps >= 0"))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const RecordRow row{counts, reinterpret_cast<const long long*>(sums), static_cast<long long>(sums_ld),
                      reinterpret_cast<const long long*>(moment_sums), source_voxel, least_points(source_min_points)};
  return gauss_newton(what, poses, n_sets, max_iteration, rot_eps, trans_eps, false, transforms, hessians, gradients, costs, nullptr, stats,
                      ws, ws_bytes, s, [&](const RegWork& w) {
                        hipLaunchKernelGGL((accumulate_kernel<false, RecordRow>), dim3(static_cast<unsigned>(n_sets * kRegGroups)),
                                           dim3(kBlock), 0, s, b.t, b.m, static_cast<long long>(capacity), voxel, row,
                                           static_cast<long long>(total), offsets, sigma * sigma, least_points(min_points), neighbors, w, 0.0);
                      });
}

// ---- voxel map queries --------------------------------------------------------------------------------------------------------

extern "C" int rdm_voxel_map_query(const void* map, size_t map_bytes, int64_t capacity, int channels, const void* moments,
                                   size_t moments_bytes, const void* observations, size_t observations_bytes, double voxel,
                                   const float* points, int64_t ld, int64_t total, const int64_t* offsets, const double* poses,
                                   int64_t n_scans, double min_range, double max_range, double sigma, int64_t min_points, int neighbors,
                                   int64_t min_scans, double max_d2, uint8_t* labels, int8_t* best, int32_t* counts, int32_t* seen,
                                   double* d2, double* d2_sum, uint8_t* pairs, int64_t* tallies, void* stream) {
  using namespace rdm;
  const char* what = "rdm_voxel_map_query";
  Blocks b;
  if (const int rc = open_blocks(what, map, map_bytes, capacity, channels, {kOptional, moments, moments_bytes},
                                 {kOptional, observations, observations_bytes}, b, RDM_ERR_ARG))
    return rc;
  if (const int rc = check_batch(what, voxel, channels, points, ld, total, offsets, poses, n_scans, INT64_MAX, false, min_range, max_range))
    return rc;
  if (const int rc = check_options(what, sigma, neighbors, min_points >= 1 && min_scans >= 0, "min_points >= 1 and min_scans >= 0")) return rc;
  RDM_REQUIRE(max_d2 >= 0.0, "%s: max_d2 must be >= 0 or +inf (got %g)", what, max_d2);  // (NaN fails)
  RDM_REQUIRE(observations != nullptr || (min_scans <= 1 && seen == nullptr),
              "%s: min_scans > 1 and the seen output need an observations block", what);
  if (n_scans == 0) return RDM_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (tallies != nullptr) fill_words<unsigned long long>(reinterpret_cast<unsigned long long*>(tallies), n_scans * kTallies, 0ull, s);
  if (total > 0) {
    // every voxel of the table was seen in at least one scan, so the records are read for min_scans > 1 or the seen output only; the
    // distances are formed where a label, the choice among seven voxels or an output needs them
    const int* records = min_scans > 1 || seen != nullptr ? b.o.record : nullptr;
    const bool dist = neighbors == 7 || max_d2 < INFINITY || d2 != nullptr || d2_sum != nullptr;
    const int64_t n_chunks = (total + kBlock - 1) / kBlock;
    const int64_t blocks = n_chunks < kQueryBlocks ? n_chunks : kQueryBlocks;
    const int64_t chunks = (n_chunks + blocks - 1) / blocks;
    const QueryOut out{labels, best, counts, seen, d2, d2_sum, pairs, reinterpret_cast<unsigned long long*>(tallies)};
    auto kernel = !dist ? query_kernel<false, false> : (b.m != nullptr ? query_kernel<true, true> : query_kernel<true, false>);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, b.t, b.m, records, static_cast<long long>(capacity),
                       channels, voxel, points, static_cast<long long>(ld), static_cast<long long>(total), offsets, poses,
                       static_cast<long long>(n_scans), min_range * min_range, max_range * max_range, sigma * sigma,
                       least_points(min_points), neighbors, static_cast<int>(min_scans > kMaxScanId ? kMaxScanId : min_scans), max_d2,
                       static_cast<long long>(chunks), out);
  }
  return launch_status(what);
}
