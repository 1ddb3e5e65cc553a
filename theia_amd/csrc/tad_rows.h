// tad_rows.h — what a row of the caller's table is and how Stage 0 judges it: the one place that decides whether a row is inside the
// time window, whether its key takes part, which lattice bucket it falls in and which error bit it raises.  Every kernel that reads the
// caller's rows (k_meta, k_scatter, k_meta_hist, k_partition, k_partition_wc, k_sparse_keys) takes its answers from here.
// Plain C++ up to the `__HIPCC__` section (a host program may include this header alone); no inline assembly.
#ifndef THEIA_TAD_ROWS_H
#define THEIA_TAD_ROWS_H

#include <stdint.h>

#include "tad_dev_err.h"   // DEV_ERR_*: what a judge raises

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TAD_ROW_FN __host__ __device__ __forceinline__
#else
#define TAD_ROW_FN inline
#endif

namespace tad {

constexpr uint64_t kKeySkip = UINT64_MAX;   // tad.h: TAD_KEY_SKIP (tad_internal.h asserts the two are one)

// flowEndSeconds lattice: t = t0 + step * bucket, bucket < nb.
struct Lattice {
  int64_t t0;
  int64_t step;
  uint64_t nb;
  uint64_t magic;  // ceil(2^64 / step): exact quotient for dividends < 2^32 (mode 1)
  int mode;        // 0: step == 1, 1: multiply-high path ((tmax - t0) < 2^32), 2: 64-bit division
};

inline Lattice make_lattice(int64_t t0, int64_t step, uint64_t nb) {
  Lattice L;
  L.t0 = t0;
  L.step = step < 1 ? 1 : step;
  L.nb = nb;
  L.magic = 0;
  if (L.step == 1) {
    L.mode = 0;
  } else {
    // ceil(2^64 / step) = floor((2^64 - 1) / step) + 1 (step >= 2 never divides 2^64 - 1 + 1 exactly
    // unless it is a power of two, for which floor((2^64-1)/step) + 1 = 2^64/step as well)
    L.magic = UINT64_MAX / (uint64_t)L.step + 1;
    // the multiply-high quotient is exact for dividends < 2^32 and divisors < 2^32
    const bool small = (uint64_t)L.step < (1ull << 32) &&
                       (nb == 0 || (nb - 1) <= (UINT32_MAX / (uint64_t)L.step));
    L.mode = small ? 1 : 2;
  }
  return L;
}

// Widths of the input columns a Stage-0 launcher reads (tad.h, TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32): 0 = every column 8 bytes.
// The kernels take them as template parameters (K32, T32) and decode on load; everything after the loads is width-independent.
enum : int { kColKey32 = 1, kColTime32 = 2 };

struct RowFilter {
  int64_t start_time;  // 0 = unset
  int64_t end_time;    // 0 = unset
};

inline bool ptr_aligned16(const void *p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The caller's table on the device.  The pointers keep their 8-byte types whatever `cw` says: a narrow column is read through
// ld_key / ld_time (tad_internal.h).
struct RowCols {
  const uint64_t *key, *key2;        // key2: NULL = one key per row
  const int64_t *t_end, *t_start;    // t_start: NULL = no flowStartSeconds column
  const uint64_t *value;
  uint64_t n;
  int cw;                            // kColKey32 | kColTime32
  bool has2() const { return key2 != nullptr; }
  bool keys_aligned16() const { return ptr_aligned16(key) && ptr_aligned16(key2) && ptr_aligned16(t_end); }   // what pass A reads
  bool aligned16() const { return keys_aligned16() && ptr_aligned16(value); }                                 // 16-byte loads of a row pair
  bool start_aligned16() const { return ptr_aligned16(t_start); }
};

// ------------------------------------------------------------------------------------------------
// the row judges
// ------------------------------------------------------------------------------------------------
TAD_ROW_FN uint64_t mul_hi_u64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the time window (has_ts: the table has a flowStartSeconds column and the job a start_time)
TAD_ROW_FN bool time_kept(int64_t te, int64_t ts, bool has_ts, RowFilter f) {
  if (f.end_time != 0 && !(te < f.end_time)) return false;                  // anomaly_detection.py:584-586
  if (f.start_time != 0 && has_ts && !(ts >= f.start_time)) return false;   // :581-583
  return true;
}

// bucket of `te` on the lattice; false = off it (before t0, past the last bucket, or between two lattice points)
TAD_ROW_FN bool lattice_bucket(const Lattice &L, int64_t te, uint64_t &bucket) {
  const uint64_t d = (uint64_t)te - (uint64_t)L.t0;  // te < t0 wraps to a huge value -> rejected below
  uint64_t b;
  if (L.mode == 0) {
    b = d;
  } else if (L.mode == 1) {
    if (d >> 32) return false;
    b = mul_hi_u64(d, L.magic);
  } else {
    b = d / (uint64_t)L.step;
  }
  if (b >= L.nb || b * (uint64_t)L.step != d) return false;
  bucket = b;
  return true;
}

// ... for a lattice of mode 0 or 1, without a branch: one multiply-high.  `bucket` is written either way (garbage off the lattice).
// Exact like the general form: mode 0 has no d < 2^32 test (pass B's fast path once had one); a caller that keeps the bucket in 32 bits
// must know nb <= 2^32 by other means — pass B does, see the casts there.
TAD_ROW_FN bool lattice_bucket_fast(const Lattice &L, int64_t te, uint64_t &bucket) {
  const uint64_t d = (uint64_t)te - (uint64_t)L.t0;
  const uint64_t bq = L.mode == 0 ? d : mul_hi_u64(d, L.magic);
  bucket = bq;
  return (L.mode == 0 || (d >> 32) == 0) && bq < L.nb && bq * (uint64_t)L.step == d;
}

TAD_ROW_FN uint64_t gcd_u64(uint64_t a, uint64_t b) {
  if (a == 0) return b;
  if (b == 0) return a;
  if (((a | b) >> 32) == 0) {
    uint32_t x = (uint32_t)a, y = (uint32_t)b;
    while (y) { uint32_t r = x % y; x = y; y = r; }
    return x;
  }
  while (b) { uint64_t r = a % b; a = b; b = r; }
  return a;
}

TAD_ROW_FN uint64_t absdiff_i64(int64_t a, int64_t b) {
  return a >= b ? (uint64_t)a - (uint64_t)b : (uint64_t)b - (uint64_t)a;
}

// Device-side counters of one run (one 64-byte block, zeroed per run): rows_used and err are what the row judges report into.
struct DevCounters {
  unsigned long long rows_used;
  unsigned long long n_keys;
  unsigned long long n_points;
  unsigned long long keys_no_result;
  unsigned long long kalman_steps;
  unsigned long long arima_fits;
  unsigned long long arima_nan_fits;   // fits whose prediction is not finite (the optimiser walked into a non-finite likelihood)
  uint32_t err;
  uint32_t pad;
};

// What a set of kept rows says about the lattice: the range of their times and g = a common divisor of every |t - tref|.
struct LatticeAcc {
  int64_t tmin, tmax, tref;
  uint64_t g, used;
};

TAD_ROW_FN LatticeAcc lattice_merge(LatticeAcc a, const LatticeAcc &b) {
  if (b.used == 0) return a;
  if (a.used == 0) return b;
  a.tmin = b.tmin < a.tmin ? b.tmin : a.tmin;
  a.tmax = b.tmax > a.tmax ? b.tmax : a.tmax;
  a.g = gcd_u64(gcd_u64(a.g, b.g), absdiff_i64(a.tref, b.tref));
  a.used += b.used;
  return a;
}

// One key slot of a row (one, or two with a second key column).  The key range comes before the lattice, whatever the row's time.
enum KeySlot : int { kSlotSkip = 0, kSlotRange = 1, kSlotLive = 2 };
TAD_ROW_FN KeySlot key_slot(bool kept, uint64_t k, uint64_t K, uint32_t &err) {
  if (!kept || k == kKeySkip) return kSlotSkip;
  if (k >= K) { err |= DEV_ERR_KEY_RANGE; return kSlotRange; }
  return kSlotLive;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ LatticeAcc lattice_shfl_down(const LatticeAcc &a, int d) {
  LatticeAcc r;
  r.tmin = __shfl_down((long long)a.tmin, d);
  r.tmax = __shfl_down((long long)a.tmax, d);
  r.tref = __shfl_down((long long)a.tref, d);
  r.g = __shfl_down((unsigned long long)a.g, d);
  r.used = __shfl_down((unsigned long long)a.used, d);
  return r;
}

// rows_used / error bits of a workgroup of kThreads: ONE atomic per workgroup.  One per wavefront was 4096 atomics on one address at the
// very end of pass B, when all workgroups finish together — contended atomics serialise at ~10 ns each.
template <int kThreads>
__device__ __forceinline__ void block_count_rows(unsigned long long used, uint32_t err, DevCounters *ctr) {
  __shared__ unsigned long long s_u[kThreads / 64];
  __shared__ uint32_t s_e[kThreads / 64];
  unsigned long long u = used;
  for (int d = 32; d >= 1; d >>= 1) { u += __shfl_down(u, d); err |= __shfl_down(err, d); }
  if ((threadIdx.x & 63) == 0) { s_u[threadIdx.x >> 6] = u; s_e[threadIdx.x >> 6] = err; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) { u += s_u[w]; err |= s_e[w]; }
    if (u) atomicAdd(&ctr->rows_used, u);
    if (err) atomicOr(&ctr->err, err);
  }
}

// ---- pass B (tad_stage0_part.hip: k_partition, k_partition_wc).  Args = PartArgs, the kernels' argument. ----

// One key slot of a row in pass B that has a record: pass A's predicate (kept, key live and in range; off the lattice: `no cell`).
struct PartSlot {
  bool sentinel;   // the record carries A.narrow_limit instead of the value (32-bit tile cells: the value is on the overflow list)
  uint32_t part;   // partition
  uint32_t cell;   // tile-local cell, all ones = no cell
};

// Judges one key slot; a reserved slot is handed to reserve(PartSlot) — once, or not at all.  The overflow-list append, the ovf_keys bit
// and the error bits happen here.  (A functor, not a returned value: k_partition<8, true, ...> runs at the 128-VGPR limit, and with the
// (reserved, part, cell, sentinel) tuple merged at a common exit it spilled 156-200 bytes per lane where this form spills 124.)
template <typename Args, typename Reserve>
__device__ __forceinline__ void part_slot(const Args &A, bool kept, bool on_lattice, uint32_t bucket, uint64_t k, uint64_t v,
                                          uint32_t &err, uint32_t &used, Reserve reserve) {
  // (pass A reports a key out of range too, but only for the rows it reads: with a sampled histogram that is one row in sixteen)
  if (key_slot(kept, k, A.K, err) != kSlotLive) return;
  uint32_t cell = (1u << A.cell_bits) - 1u;
  bool sentinel = false;
  if (on_lattice) {
    used++;
    const bool big = v >= A.value_limit || (A.narrow_limit != 0 && v >= A.narrow_limit);
    if (!big || A.narrow_limit != 0) cell = bucket * (A.kp_mask + 1u) + ((uint32_t)k & A.kp_mask);
    if (big) {  // rare: the value does not fit the record (or the 32-bit tile cell) -> overflow list
      const unsigned long long o = atomicAdd(A.ovf_count, 1ull);
      if (o < A.ovf_cap) { A.ovf[o].val = v; A.ovf[o].gcell = (unsigned long long)bucket * A.K + k; }
      else err |= DEV_ERR_OVERFLOW_LIST;
      if (A.ovf_keys != nullptr) atomicOr(A.ovf_keys + (k >> 5), 1u << (k & 31u));
      sentinel = A.narrow_limit != 0;      // the record stays, with the sentinel value: the tile cell becomes all ones
    }
  } else {
    err |= DEV_ERR_OFF_LATTICE;            // wrong lattice hint, or the sampled gcd missed a residue: host re-derives
  }
  reserve(PartSlot{sentinel, (uint32_t)(k >> A.shift_part), cell});
}

template <typename Args>
__device__ __forceinline__ unsigned long long part_record(const Args &A, uint64_t v, uint32_t cell, bool sentinel) {
  return ((sentinel ? A.narrow_limit : (unsigned long long)v) << A.cell_bits) | cell;
}

// The prologue of a pass-B workgroup: the cursors of its F regions in LDS (gcur: next record slot, gend: end of the region), and whether
// the workgroup has nothing to do — k_part_offsets found that the sampled layout does not suit this table and the host redoes the job
// with the exact histogram.  That answer is `*s_shut`: ONE thread reads A.ctr->err and publishes the word through LDS; every thread
// branches on it behind the caller's next barrier (`if (*s_shut) return;`), so that the workgroup leaves whole or not at all.  The bit is
// also raised by other pass-B workgroups as they finish: were it tested per thread, a workgroup that starts late could lose some of its
// wavefronts and go on with cursors that the loop below — which strides over all threads — had only partly written.
// The flag load stays out of the tile loop (vmcnt retires in order: waiting for one fresh load waits for every prefetched row behind it).
template <int kThreads, typename Args>
__device__ __forceinline__ void regions_open(const Args &A, int G, uint32_t F, uint32_t *gcur, uint32_t *gend, uint32_t *s_shut) {
  if (threadIdx.x == 0) *s_shut = (A.fin != nullptr && (A.ctr->err & DEV_ERR_REGION_FULL)) ? 1u : 0u;
  const uint32_t *my = A.offs32 + (size_t)blockIdx.x * F;
  const uint32_t *nx = A.offs32 + (size_t)(blockIdx.x + 1) * F;
  const bool last = (int)blockIdx.x + 1 == G;      // G: workgroups of the pass
  for (uint32_t p = threadIdx.x; p < F; p += kThreads) {
    const uint32_t ps = (uint32_t)A.part_start[p];
    gcur[p] = ps + my[p];
    gend[p] = last ? (uint32_t)A.part_start[p + 1] : ps + nx[p];
  }
}

// sampled regions: where region (this workgroup, p) ends its upward records and starts its spilled ones
template <typename Args>
__device__ __forceinline__ void regions_fin(const Args &A, uint32_t F, uint32_t p, uint32_t up_end, uint32_t spill_start) {
  uint32_t *fo = A.fin + ((size_t)blockIdx.x * F + p) * 2;
  fo[0] = up_end;
  fo[1] = spill_start;
}
#endif  // __HIPCC__

}  // namespace tad

#endif  // THEIA_TAD_ROWS_H
