// tad_history.hip — the per-key value history of a streaming state (include/tad.h: TAD_STATE_HISTORY) and the streaming DBSCAN
// verdicts judged against it.
//
// A history state keeps, per key, every aggregated point value it has seen, sorted ascending as UInt64 (u64 -> f64 is monotone, so
// u64 order is f64 order): hist_off[K + 1] and hist_val[].  One batch of tad_run_stream on such a state:
//   1. the batch's new points in (key, time) order: nk / nt / nv with poff[K + 1] (k_hist_decode for a sparse batch; a dense one is
//      compacted by launch_count_flags + launch_scan + launch_emit_points);
//   2. the key's new values sorted (k_hist_sort_wave: a wavefront per key, bitonic in registers for <= 64 points; longer segments go to
//      k_hist_sort_long: a workgroup per key, bitonic in LDS for <= kHistLdsPoints points, in place in global memory beyond);
//   3. old and new merged into the candidate arena (k_hist_chunks + launch_scan + k_hist_merge: every element finds its place by one
//      binary search in the other segment, so a key's merge is split over as many wavefronts as it has chunks of kHistChunk elements);
//   4. one lane per new point: the DBSCAN noise predicate against the key's merged segment (k_hist_verdict);
//   5. the rows of the new points in (key, time) order (launch_scan over the per-point row counts, k_hist_emit).
// The noise predicate is tad_dbscan.hip's: core(x) <=> #{j : fl|x - x_j| <= eps} >= min_samples, noise(x) <=> not
// core and no core point within eps.  It depends only on the multiset of the key's values, so judging a new point against the merged
// history gives the batch job's verdict over the concatenated table, bit for bit.
#include <stdint.h>

#include "tad_internal.h"

namespace tad {

static constexpr int kHBlock = 256;
static constexpr int kHWaves = kHBlock / 64;
static constexpr uint32_t kHistLdsPoints = 4096;   // k_hist_sort_long: segments up to this many points sort in LDS (32 KB)

// ---- 1. the sparse batch's sorted unique points (comp = key << 32 | (t - t0)) as key / time columns ----
__global__ __launch_bounds__(kHBlock) void k_hist_decode(const unsigned long long *__restrict__ comp, uint64_t P, int64_t t0,
                                                        unsigned long long *__restrict__ nk, long long *__restrict__ nt) {
  const uint64_t i = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= P) return;
  const unsigned long long c = comp[i];
  nk[i] = c >> 32;
  nt[i] = (long long)(t0 + (int64_t)(c & 0xffffffffull));
}

// ---- 2. sort every key's new values ----
// One wavefront per key: segments of <= 64 values sort in registers (bitonic by xor-shuffle, padded with UINT64_MAX); longer ones are
// listed for k_hist_sort_long.  ns = the sorted copy of nv, same offsets.
__global__ __launch_bounds__(kHBlock) void k_hist_sort_wave(const unsigned long long *__restrict__ nv, const unsigned long long *__restrict__ poff,
                                                           uint64_t K, unsigned long long *__restrict__ ns, uint32_t *__restrict__ long_list,
                                                           unsigned int *__restrict__ long_count) {
  const uint64_t k = ((uint64_t)blockIdx.x * kHBlock + threadIdx.x) >> 6;   // wavefront-uniform
  if (k >= K) return;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  if (b == 0) return;
  if (b > 64) {
    if (lane == 0) long_list[atomicAdd(long_count, 1u)] = (uint32_t)k;
    return;
  }
  unsigned long long v = lane < b ? nv[p0 + lane] : ~0ull;
  for (unsigned kk = 2; kk <= 64; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      const unsigned long long o = __shfl_xor(v, (int)j);
      const bool up = (lane & kk) == 0, lower = (lane & j) == 0;
      v = (lower == up) ? (v < o ? v : o) : (v < o ? o : v);
    }
  if (lane < b) ns[p0 + lane] = v;
}

// Bitonic sort of a[0, n) ascending with every comparator ascending (the "flip" form: the first step of each merge compares mirrored
// positions): an index >= n would hold +inf and never move, so those comparators are skipped and n need not be a power of two.
// Called by the whole workgroup; a is LDS or global memory (the workgroup's barriers order both).
__device__ __forceinline__ void bitonic_flip(unsigned long long *a, uint32_t n) {
  uint32_t np2 = 1;
  while (np2 < n) np2 <<= 1;
  const uint32_t half = np2 >> 1;
  for (uint32_t kk = 2; kk <= np2; kk <<= 1) {
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      const bool flip = j == (kk >> 1);
      for (uint32_t i = threadIdx.x; i < half; i += kHBlock) {
        const uint32_t i1 = (i / j) * (2 * j) + (i % j);
        const uint32_t i2 = flip ? (i1 | (kk - 1)) - (i1 & (kk - 1)) : i1 + j;   // flip: the mirror of i1 inside its block of kk
        if (i2 < n) {
          const unsigned long long x = a[i1], y = a[i2];
          if (y < x) { a[i1] = y; a[i2] = x; }
        }
      }
      __syncthreads();
    }
  }
}

// One workgroup per listed key (grid-stride over the list): the segment is copied to ns and sorted there — through LDS when it fits,
// else in place in global memory (a key with more than kHistLdsPoints points in ONE batch: over an hour of seconds).
__global__ __launch_bounds__(kHBlock) void k_hist_sort_long(const unsigned long long *__restrict__ nv, const unsigned long long *__restrict__ poff,
                                                           unsigned long long *__restrict__ ns, const uint32_t *__restrict__ long_list,
                                                           const unsigned int *__restrict__ long_count) {
  __shared__ unsigned long long s_v[kHistLdsPoints];
  const unsigned total = *long_count;
  for (unsigned e = blockIdx.x; e < total; e += gridDim.x) {
    const uint64_t k = long_list[e];
    const unsigned long long p0 = poff[k];
    const uint32_t b = (uint32_t)(poff[k + 1] - p0);
    const bool lds = b <= kHistLdsPoints;
    unsigned long long *a = lds ? s_v : ns + p0;
    for (uint32_t i = threadIdx.x; i < b; i += kHBlock) a[i] = nv[p0 + i];
    __syncthreads();
    bitonic_flip(a, b);
    if (lds)
      for (uint32_t i = threadIdx.x; i < b; i += kHBlock) ns[p0 + i] = s_v[i];
    __syncthreads();
  }
}

// ---- 3. merge old and new into the candidate arena ----
// hist_new_off[k] = hist_old_off[k] + poff[k] (the exclusive scan of old + new lengths is the sum of the two scans); chunks[k] = the key's
// wavefronts in k_hist_merge.
__global__ __launch_bounds__(kHBlock) void k_hist_chunks(const unsigned long long *__restrict__ hoff_old, const unsigned long long *__restrict__ poff,
                                                        uint64_t K, unsigned long long *__restrict__ hoff_new, uint32_t *__restrict__ chunks) {
  const uint64_t k = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (k > K) return;
  hoff_new[k] = hoff_old[k] + poff[k];
  if (k == K) return;
  const unsigned long long len = (hoff_old[k + 1] - hoff_old[k]) + (poff[k + 1] - poff[k]);
  chunks[k] = (uint32_t)((len + kHistChunk - 1) / kHistChunk);
}

// lower_bound / upper_bound of v in the ascending a[lo, hi): the first index whose value is >= v (> v)
__device__ __forceinline__ unsigned long long lower_u64(const unsigned long long *a, unsigned long long lo, unsigned long long hi, unsigned long long v) {
  while (lo < hi) { const unsigned long long mid = lo + ((hi - lo) >> 1); if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ unsigned long long upper_u64(const unsigned long long *a, unsigned long long lo, unsigned long long hi, unsigned long long v) {
  while (lo < hi) { const unsigned long long mid = lo + ((hi - lo) >> 1); if (a[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}

// One wavefront per chunk: the chunk's key from the chunk offsets (binary search, wavefront-uniform), then every element of the key's
// [old segment | new segment] in the chunk goes to its merged place: old[i] -> i + #{new < old[i]}, new[j] -> j + #{old <= new[j]}
// (a stable merge, old first on ties).  A key without new points is a coalesced copy.
__global__ __launch_bounds__(kHBlock) void k_hist_merge(const unsigned long long *__restrict__ coff, uint64_t K,
                                                       const unsigned long long *__restrict__ hoff_old, const unsigned long long *__restrict__ hval_old,
                                                       const unsigned long long *__restrict__ poff, const unsigned long long *__restrict__ ns,
                                                       const unsigned long long *__restrict__ hoff_new, unsigned long long *__restrict__ hval_new) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kHBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  uint64_t lo = 0, hi = K;   // the last key k with coff[k] <= w (a key with chunks has coff[k] < coff[k + 1])
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (coff[mid] <= w) lo = mid; else hi = mid; }
  const uint64_t k = lo;
  const unsigned long long o0 = hoff_old[k], a = hoff_old[k + 1] - o0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  const unsigned long long dst0 = hoff_new[k];
  const unsigned long long c0 = (w - coff[k]) * kHistChunk;
  unsigned long long c1 = c0 + kHistChunk;
  if (c1 > a + b) c1 = a + b;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    if (u < a) {
      const unsigned long long x = hval_old[o0 + u];
      const unsigned long long r = b ? lower_u64(ns, p0, p0 + b, x) - p0 : 0ull;
      hval_new[dst0 + u + r] = x;
    } else {
      const unsigned long long j = u - a, y = ns[p0 + j];
      const unsigned long long r = upper_u64(hval_old, o0, o0 + a, y) - o0;
      hval_new[dst0 + j + r] = y;
    }
  }
}

// ---- 4. verdicts ----
// h[s0, s1) = the key's merged values (ascending).  The window of h[p] inside [lo_cap, hi_cap]: binary searches with the very predicate
// of the pair test, fl|x_p - x_m| <= eps, which is monotone on either side of p (tad_dbscan.hip:k_dbscan_sorted).
struct Window { unsigned long long lo, hi; };
__device__ __forceinline__ Window hist_window(const unsigned long long *h, unsigned long long p, unsigned long long lo_cap, unsigned long long hi_cap,
                                             double eps) {
  const double x = (double)h[p];
  unsigned long long a = lo_cap, b = p;        // false ... false true ... true on [lo_cap, p]
  while (a < b) { const unsigned long long mid = (a + b) >> 1; if (fabs(x - (double)h[mid]) <= eps) b = mid; else a = mid + 1; }
  const unsigned long long l = a;
  a = p; b = hi_cap;                            // true ... true false ... false on [p, hi_cap]
  while (a < b) { const unsigned long long mid = (a + b + 1) >> 1; if (fabs(x - (double)h[mid]) <= eps) a = mid; else b = mid - 1; }
  return Window{l, a};
}

// the window of h[p] capped to min_samples points on either side of p: it holds >= ms points exactly when the full window does
// (a full window of >= ms points contains ms consecutive indices around p), and is the full window when that has fewer
__device__ __forceinline__ Window hist_window_capped(const unsigned long long *h, unsigned long long p, unsigned long long s0, unsigned long long s1,
                                                    uint32_t ms, double eps) {
  const unsigned long long r = ms - 1u;
  const unsigned long long lo_cap = p - s0 >= r ? p - r : s0;
  const unsigned long long hi_cap = s1 - 1 - p >= r ? p + r : s1 - 1;
  return hist_window(h, p, lo_cap, hi_cap, eps);
}

// One lane per new point, in (key, time) order.  noise[i] = the verdict; cnt[i] = the rows the point emits (all_points: 1; else the
// verdict); lanes in [P, P_cap) write cnt = 0 so that the scan may run over the host's bound P_cap.
__global__ __launch_bounds__(kHBlock) void k_hist_verdict(const unsigned long long *__restrict__ nk, const unsigned long long *__restrict__ nv,
                                                         const unsigned long long *__restrict__ P_dev, uint64_t P_cap,
                                                         const unsigned long long *__restrict__ hoff, const unsigned long long *__restrict__ h,
                                                         double eps, uint32_t ms, bool all_points, uint8_t *__restrict__ noise,
                                                         uint32_t *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= P_cap) return;
  if (i >= *P_dev) { cnt[i] = 0; return; }
  const uint64_t k = nk[i];
  const unsigned long long raw = nv[i], s0 = hoff[k], s1 = hoff[k + 1];
  bool z;
  if (s1 - s0 < ms) z = true;                                            // no point of the key can be core yet
  else if ((double)h[s1 - 1] - (double)h[s0] <= eps) z = false;          // k_dbscan_scan's settle rule: every pair within eps
  else {
    const unsigned long long p = lower_u64(h, s0, s1, raw);             // h[p] == raw: the point is in the merged segment
    const Window w = hist_window_capped(h, p, s0, s1, ms, eps);
    z = w.hi - w.lo + 1 < ms;
    for (unsigned long long m = w.lo; z && m <= w.hi; ++m) {            // fewer than ms neighbours: noise unless one of them is core
      if (h[m] == raw) continue;                                        // (same value, same window: not core either)
      const Window wm = hist_window_capped(h, m, s0, s1, ms, eps);
      if (wm.hi - wm.lo + 1 >= ms) z = false;
    }
  }
  noise[i] = z ? 1 : 0;
  cnt[i] = (all_points || z) ? 1u : 0u;
}

// ---- 5. rows ----
// Row row[i] for every point with cnt[i] != 0: key, time, float(value), algoCalc 0.0 (anomaly_detection.py:312-322) and the key's
// stddev_samp over everything seen, from the candidate moments by k_emit<4>'s final expression.
__global__ __launch_bounds__(kHBlock) void k_hist_emit(const unsigned long long *__restrict__ nk, const long long *__restrict__ nt,
                                                      const unsigned long long *__restrict__ nv, const unsigned long long *__restrict__ P_dev,
                                                      const uint8_t *__restrict__ noise, const uint32_t *__restrict__ cnt,
                                                      const unsigned long long *__restrict__ row, StreamState next, bool all_points, OutRows out) {
  const uint64_t i = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (i >= *P_dev || cnt[i] == 0) return;
  const uint64_t k = nk[i];
  const unsigned long long at = row[i];
  const uint32_t n = next.n[k];
  const double s_cnt = (double)n;
  const double sg = n >= 2 ? sqrt(next.m2[k] / (s_cnt - 1.0)) : 0.0;
  out.key_id[at] = k;
  out.flow_end_s[at] = nt[i];
  out.throughput[at] = (double)nv[i];
  out.algo_calc[at] = 0.0;
  out.stddev[at] = sg;
  if (all_points) out.anomaly[at] = noise[i];
}

// ---- launchers ----
static inline unsigned hist_blocks(uint64_t lanes) { return (unsigned)((lanes + kHBlock - 1) / kHBlock); }

void launch_hist_decode(hipStream_t s, const unsigned long long *comp, uint64_t P, int64_t t0, unsigned long long *nk, long long *nt) {
  if (P == 0) return;
  hipLaunchKernelGGL(k_hist_decode, dim3(hist_blocks(P)), dim3(kHBlock), 0, s, comp, P, t0, nk, nt);
}

void launch_hist_sort(hipStream_t s, const unsigned long long *nv, const unsigned long long *poff, uint64_t K, unsigned long long *ns,
                      uint32_t *long_list, unsigned int *long_count) {
  if (K == 0) return;
  hipMemsetAsync(long_count, 0, sizeof(unsigned int), s);
  hipLaunchKernelGGL(k_hist_sort_wave, dim3(hist_blocks(K * 64)), dim3(kHBlock), 0, s, nv, poff, K, ns, long_list, long_count);
  const unsigned g = (unsigned)(K < 2048 ? K : 2048);
  hipLaunchKernelGGL(k_hist_sort_long, dim3(g), dim3(kHBlock), 0, s, nv, poff, ns, long_list, long_count);
}

uint64_t hist_merge_chunks_bound(uint64_t K, uint64_t total_len) { return K + total_len / kHistChunk + 1; }

void launch_hist_merge(hipStream_t s, uint64_t K, const unsigned long long *hoff_old, const unsigned long long *hval_old, const unsigned long long *poff,
                       const unsigned long long *ns, unsigned long long *hoff_new, unsigned long long *hval_new, uint32_t *chunks,
                       unsigned long long *coff, unsigned long long *scan_scratch, uint64_t chunks_bound) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_hist_chunks, dim3(hist_blocks(K + 1)), dim3(kHBlock), 0, s, hoff_old, poff, K, hoff_new, chunks);
  launch_scan(s, chunks, coff, K, scan_scratch);
  hipLaunchKernelGGL(k_hist_merge, dim3(hist_blocks(chunks_bound * 64)), dim3(kHBlock), 0, s, coff, K, hoff_old, hval_old, poff, ns, hoff_new, hval_new);
}

void launch_hist_verdict(hipStream_t s, const unsigned long long *nk, const unsigned long long *nv, const unsigned long long *P_dev, uint64_t P_cap,
                         const unsigned long long *hoff, const unsigned long long *h, double eps, int min_samples, bool all_points, uint8_t *noise,
                         uint32_t *cnt) {
  if (P_cap == 0) return;
  hipLaunchKernelGGL(k_hist_verdict, dim3(hist_blocks(P_cap)), dim3(kHBlock), 0, s, nk, nv, P_dev, P_cap, hoff, h, eps, (uint32_t)min_samples, all_points,
                     noise, cnt);
}

void launch_hist_emit(hipStream_t s, const unsigned long long *nk, const long long *nt, const unsigned long long *nv, const unsigned long long *P_dev,
                      uint64_t P_cap, const uint8_t *noise, const uint32_t *cnt, const unsigned long long *row, StreamState next, bool all_points,
                      OutRows out) {
  if (P_cap == 0) return;
  hipLaunchKernelGGL(k_hist_emit, dim3(hist_blocks(P_cap)), dim3(kHBlock), 0, s, nk, nt, nv, P_dev, noise, cnt, row, next, all_points, out);
}

// ---- the series of a streaming state (TAD_STATE_SERIES): every key's values in time order ----
// A batch's new points are later than everything its key has seen (a late row fails the batch), so the candidate series of key k is
// its old segment followed by its new points: soff_new[k] = soff_old[k] + poff[k], then one wavefront per key copies both.
__global__ __launch_bounds__(kHBlock) void k_series_off(const unsigned long long *__restrict__ soff_old, const unsigned long long *__restrict__ poff,
                                                       uint64_t K, unsigned long long *__restrict__ soff_new) {
  const uint64_t k = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (k <= K) soff_new[k] = soff_old[k] + poff[k];
}

__global__ __launch_bounds__(kHBlock) void k_series_append(uint64_t K, const unsigned long long *__restrict__ soff_old,
                                                          const unsigned long long *__restrict__ sval_old, const unsigned long long *__restrict__ poff,
                                                          const unsigned long long *__restrict__ nv, const unsigned long long *__restrict__ soff_new,
                                                          unsigned long long *__restrict__ sval_new) {
  const uint64_t k = ((uint64_t)blockIdx.x * kHBlock + threadIdx.x) >> 6;   // wavefront-uniform
  if (k >= K) return;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long o0 = soff_old[k], a = soff_old[k + 1] - o0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  unsigned long long *dst = sval_new + soff_new[k];
  for (unsigned long long u = lane; u < a; u += 64) dst[u] = sval_old[o0 + u];
  for (unsigned long long u = lane; u < b; u += 64) dst[a + u] = nv[p0 + u];
}

void launch_series_append(hipStream_t s, uint64_t K, const unsigned long long *soff_old, const unsigned long long *sval_old, const unsigned long long *poff,
                          const unsigned long long *nv, unsigned long long *soff_new, unsigned long long *sval_new) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_series_off, dim3(hist_blocks(K + 1)), dim3(kHBlock), 0, s, soff_old, poff, K, soff_new);
  hipLaunchKernelGGL(k_series_append, dim3(hist_blocks(K * 64)), dim3(kHBlock), 0, s, K, soff_old, sval_old, poff, nv, soff_new, sval_new);
}

// ---- tad_state_trim: drop every key's oldest points (include/tad.h) ----
// A series state keeps key k's points in time order at soff[k], times (TAD_STATE_TIMES) alongside, and its history holds the same
// values sorted; a trim keeps a suffix of every key's series:
//   1. k_trim_keep, one lane per key: the time cut (lower_bound of keep_from in the key's times), then at most keep_points of the rest.
//      rcnt[k] = retained, ecnt[k] = evicted, chunks[k] = the key's wavefronts in 2 / 4 (old segment length / kHistChunk).
//   2. the retained suffix of every key's values (and times) into the candidate arena, the evicted prefix packed for the history
//      (k_trim_copy, a wavefront per chunk as k_hist_merge: coalesced, and a key of a day of seconds is 43 wavefronts, not one).
//   3. a history state: the evicted prefixes sorted per key (launch_hist_sort), then
//   4. k_hist_subtract removes them from the history: one lane per history element, chunked like 2 (a key's history is as long as its
//      series).  Element h[i] = v with rank r inside its run of equal values and c copies of v among the key's evicted values: kept iff
//      r >= c, at i - #{evicted < v} - min(r, c).  The cost follows the history plus the evicted points; the retained series is not
//      re-sorted.
//   5. k_trim_moments, one lane per key: a key that lost points replays stream_step over its retained values from the zero state (the
//      fresh state's moments bit for bit: the same inline step, the same order); a key that lost all is unseen; the others are copied.
__global__ __launch_bounds__(kHBlock) void k_trim_keep(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                      uint64_t keep_points, long long keep_from, uint32_t *__restrict__ rcnt,
                                                      uint32_t *__restrict__ ecnt, uint32_t *__restrict__ chunks) {
  const uint64_t k = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (k >= K) return;
  const unsigned long long o0 = soff[k], len = soff[k + 1] - o0;
  unsigned long long lo = 0;
  if (st) {   // the first point at or after keep_from (times ascend)
    unsigned long long hi = len;
    while (lo < hi) { const unsigned long long mid = lo + ((hi - lo) >> 1); if (st[o0 + mid] < keep_from) lo = mid + 1; else hi = mid; }
  }
  unsigned long long r = len - lo;
  if (keep_points && r > keep_points) r = keep_points;
  rcnt[k] = (uint32_t)r;
  ecnt[k] = (uint32_t)(len - r);
  chunks[k] = len > kHistChunk ? (uint32_t)((len + kHistChunk - 1) / kHistChunk) : 1u;   // (an empty key too: see chunk_key_min1)
}

// One wavefront per chunk of a key's OLD segment: element u < e goes to the packed evicted values (ev at eoff[k], history states only),
// element u >= e to the candidate series at soff_new[k] + u - e (values, and times when st_old is given).
__global__ __launch_bounds__(kHBlock) void k_trim_copy(const unsigned long long *__restrict__ coff, uint64_t K,
                                                      const unsigned long long *__restrict__ soff_old, const unsigned long long *__restrict__ sval_old,
                                                      const long long *__restrict__ st_old, const unsigned long long *__restrict__ soff_new,
                                                      unsigned long long *__restrict__ sval_new, long long *__restrict__ st_new,
                                                      const unsigned long long *__restrict__ eoff, unsigned long long *__restrict__ ev) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kHBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key_min1(coff, K, w);   // (coff: the scan of k_trim_keep's chunks)
  const unsigned long long o0 = soff_old[k], len = soff_old[k + 1] - o0;
  const unsigned long long d0 = soff_new[k], e = len - (soff_new[k + 1] - d0);
  const unsigned long long c0 = (w - coff[k]) * kHistChunk;
  unsigned long long c1 = c0 + kHistChunk;
  if (c1 > len) c1 = len;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    const unsigned long long x = sval_old[o0 + u];
    if (u >= e) {
      sval_new[d0 + u - e] = x;
      if (st_old) st_new[d0 + u - e] = st_old[o0 + u];
    } else if (ev) {
      ev[eoff[k] + u] = x;
    }
  }
}

// One wavefront per chunk of a key's old history (the chunks of its series: the same length); es = the key's evicted values sorted at
// [eoff[k], eoff[k + 1]); hoff_new = the candidate series offsets (retained history = retained series, key by key).  kMin1: the chunk
// counts give every key at least one chunk (a trim's, a window's; not a merge's, whose empty keys have none): see chunk_key_min1.
template <bool kMin1>
__global__ __launch_bounds__(kHBlock) void k_hist_subtract(const unsigned long long *__restrict__ coff, uint64_t K,
                                                          const unsigned long long *__restrict__ hoff_old, const unsigned long long *__restrict__ hval_old,
                                                          const unsigned long long *__restrict__ eoff, const unsigned long long *__restrict__ es,
                                                          const unsigned long long *__restrict__ hoff_new, unsigned long long *__restrict__ hval_new) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kHBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = kMin1 ? chunk_key_min1(coff, K, w) : chunk_key(coff, K, w);
  const unsigned long long o0 = hoff_old[k], len = hoff_old[k + 1] - o0;
  const unsigned long long e0 = eoff[k], e1 = eoff[k + 1];
  unsigned long long *dst = hval_new + hoff_new[k];
  const unsigned long long rlen = hoff_new[k + 1] - hoff_new[k];
  const unsigned long long c0 = (w - coff[k]) * kHistChunk;
  unsigned long long c1 = c0 + kHistChunk;
  if (c1 > len) c1 = len;
  for (unsigned long long i = c0 + lane; i < c1; i += 64) {
    const unsigned long long v = hval_old[o0 + i];
    if (e0 == e1) { dst[i] = v; continue; }   // the key lost nothing: a coalesced copy
    // the evicted list first: most elements have no evicted copy (c == 0: kept, whatever the rank) and skip the search for their rank
    const unsigned long long lt = lower_u64(es, e0, e1, v), c = upper_u64(es, lt, e1, v) - lt;
    const unsigned long long r = c == 0 ? 0ull : i - (lower_u64(hval_old, o0, o0 + len, v) - o0);
    const unsigned long long drop = (lt - e0) + c;   // (min(r, c) = c for a kept element)
    if (r >= c && i >= drop && i - drop < rlen) dst[i - drop] = v;   // (the bounds hold whenever the evicted values are in the history)
  }
}

static constexpr int kTrimChunk = 8;   // points per prefetched register chunk of k_trim_moments (64 B of values)
// One lane per key: the candidate moments.  The retained values are read from the candidate series (written by k_trim_copy);
// last_t stays: a key that keeps a point keeps its newest one.  NEW_T (tad_state_rollup, where a key's newest point can move to its
// bucket's start): last_t of every key with a point is the candidate times' last entry of the key, whether the key lost a point or not.
template <typename... NEW_T>   // (no argument: the trim's kernel with the trim's arguments; one: const long long *st_new)
__global__ __launch_bounds__(kHBlock) void k_trim_moments(uint64_t K, const uint32_t *__restrict__ rcnt, const uint32_t *__restrict__ ecnt,
                                                         const unsigned long long *__restrict__ soff_new, const unsigned long long *__restrict__ sval_new,
                                                         double alpha, StreamState cur, StreamState next, NEW_T... st_new) {
  const uint64_t k = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
  if (k >= K) return;
  StreamAcc a = stream_load(cur, k);
  const uint32_t r = rcnt[k];
  if (ecnt[k] != 0) {
    const long long last_t = a.last_t;
    a = StreamAcc{0u, 0.0, 0.0, 0.0, 0.0, 0ll, false};
    if (r != 0) {
      // the values in chunks of kTrimChunk, prefetched two ahead (k_win_ewma's scheme): the loads do not wait for the FP64 chain
      const double one_minus = 1.0 - alpha;
      const unsigned long long p0 = soff_new[k], len = r;
      const unsigned long long nch = (len + kTrimChunk - 1) / kTrimChunk;
      unsigned long long va[kTrimChunk], vb[kTrimChunk];
      auto load = [&](unsigned long long c, unsigned long long *v) {   // (an index past the end re-reads the last point: in bounds)
#pragma unroll
        for (int u = 0; u < kTrimChunk; ++u) {
          const unsigned long long i = c * kTrimChunk + u;
          v[u] = sval_new[p0 + (i < len ? i : len - 1)];
        }
      };
      auto consume = [&](unsigned long long c, const unsigned long long *v) {
#pragma unroll
        for (int u = 0; u < kTrimChunk; ++u) {
          if (c * kTrimChunk + u >= len) break;
          double sg;
          (void)stream_step(a, alpha, one_minus, (double)v[u], last_t, &sg);
        }
      };
      load(0, va);
      for (unsigned long long c = 0; c < nch; c += 2) {
        load(c + 1 < nch ? c + 1 : c, vb);
        consume(c, va);
        load(c + 2 < nch ? c + 2 : nch - 1, va);
        if (c + 1 < nch) consume(c + 1, vb);
      }
    }
  }
  if constexpr (sizeof...(NEW_T) != 0) {
    const long long *const t_new[] = {st_new...};
    if (r != 0) a.last_t = t_new[0][soff_new[k] + r - 1];
  }
  stream_store(next, k, a);
}

uint64_t trim_chunks_bound(uint64_t K, uint64_t total_len) { return K + total_len / kHistChunk + 1; }

void launch_trim_keep(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, uint64_t keep_points, long long keep_from,
                      uint32_t *rcnt, uint32_t *ecnt, uint32_t *chunks) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_trim_keep, dim3(hist_blocks(K)), dim3(kHBlock), 0, s, K, soff, st, keep_points, keep_from, rcnt, ecnt, chunks);
}

void launch_trim_copy(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const unsigned long long *soff_old,
                      const unsigned long long *sval_old, const long long *st_old, const unsigned long long *soff_new, unsigned long long *sval_new,
                      long long *st_new, const unsigned long long *eoff, unsigned long long *ev) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_trim_copy, dim3(hist_blocks(chunks_bound * 64)), dim3(kHBlock), 0, s, coff, K, soff_old, sval_old, st_old, soff_new, sval_new,
                     st_new, eoff, ev);
}

void launch_hist_subtract(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const unsigned long long *hoff_old,
                          const unsigned long long *hval_old, const unsigned long long *eoff, const unsigned long long *es,
                          const unsigned long long *hoff_new, unsigned long long *hval_new, bool chunks_min1) {
  if (K == 0) return;
  const dim3 grid(hist_blocks(chunks_bound * 64)), block(kHBlock);
  if (chunks_min1) hipLaunchKernelGGL(k_hist_subtract<true>, grid, block, 0, s, coff, K, hoff_old, hval_old, eoff, es, hoff_new, hval_new);
  else hipLaunchKernelGGL(k_hist_subtract<false>, grid, block, 0, s, coff, K, hoff_old, hval_old, eoff, es, hoff_new, hval_new);
}

void launch_trim_moments(hipStream_t s, uint64_t K, const uint32_t *rcnt, const uint32_t *ecnt, const unsigned long long *soff_new,
                         const unsigned long long *sval_new, double alpha, StreamState cur, StreamState next) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_trim_moments<>, dim3(hist_blocks(K)), dim3(kHBlock), 0, s, K, rcnt, ecnt, soff_new, sval_new, alpha, cur, next);
}

void launch_rollup_moments(hipStream_t s, uint64_t K, const uint32_t *rcnt, const uint32_t *ecnt, const unsigned long long *soff_new,
                           const unsigned long long *sval_new, const long long *st_new, double alpha, StreamState cur, StreamState next) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_trim_moments<const long long *>, dim3(hist_blocks(K)), dim3(kHBlock), 0, s, K, rcnt, ecnt, soff_new, sval_new, alpha, cur, next, st_new);
}

const void *code_anchor_history() { return reinterpret_cast<const void *>(&k_hist_verdict); }

}  // namespace tad
