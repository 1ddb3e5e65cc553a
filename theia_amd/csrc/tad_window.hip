// tad_window.hip — the batch verdicts of a streaming state's whole window, computed from the state alone (include/tad.h: tad_run_state).
//
// A state with a series and times holds what Stage 0 would produce for the window: ser_off[K + 1], ser_val[] and ser_t[] are every
// key's aggregated points in time order (CSR, key-major), the moments (n, avg, m2) are the batch job's bit for bit.  The grid kernels
// of tad_kernels.hip walk a time-major grid and do not apply; these walk the CSR arrays:
//   k_win_route      the keys long enough for a wavefront of their own, listed (ballot-compacted: one atomic per wavefront), and the
//                    smallest retained time (tad_stats.t0);
//   k_win_ewma       one lane per key: the EWMA recurrence replayed from 0 over the key's segment, verdict against the stddev_samp of
//                    the WHOLE series (from the state's moments, k_key_sigma's final expression).  Every lane prefetches its next two
//                    chunks of kWinChunk points into registers before it consumes one, so a wavefront keeps 64 x 2 x 64 B of its own
//                    segments in flight instead of one point per lane (k_stream_points: one exposed round trip per point);
//   k_win_emit_staged  the emit pass of k_win_ewma for anomalous rows only, with COALESCED row stores (k_emit_staged's scheme on the CSR
//                    series): one wavefront = 64 consecutive keys, whose rows are ONE contiguous range [off[k0], off[k0 + 64]) of every
//                    output column.  During the walk a lane parks (e_t, point, lane) of each anomalous point in LDS at its row's place
//                    inside that range (13 B a row); afterwards the wavefront writes the range row by row, five coalesced stores per 64
//                    rows, value and time re-read from the series (an L2 / MALL hit: the wavefront has just walked it).  Rows past the
//                    LDS capacity are stored directly, as k_win_ewma does, so any capacity is correct;
//   k_win_ewma_coop  one wavefront per listed key (walk_series_coop's scheme on a contiguous segment): lane l loads point 64 c + l,
//                    three blocks in flight, all lanes step on readlane broadcasts; lane u keeps the EWMA value and verdict of point
//                    u, so the rows of a block are written by their own lanes, coalesced;
//   k_win_keys       the key of every series point (what launch_hist_verdict / launch_hist_emit / launch_as_emit index by).
// The count pass (EMIT = false) leaves n_anom[k]; the emit pass replays and writes rows at off[k].  With TAD_FLAG_EMIT_ALL_POINTS the
// row offsets are ser_off itself and the count pass is skipped.  The recurrence is the sequential one of k_key_sigma / k_emit —
// e = one_minus * e + alpha * x, x = (double)value, in time order — so the bits are theirs.
#include <stdint.h>

#include "tad_internal.h"
#include "tad_bucket.h"

namespace tad {

static constexpr int kWBlock = 256;
static constexpr int kWinChunk = 8;   // points per lane and prefetch (64 B of values)

__device__ __forceinline__ double win_sigma(const StreamState &cur, uint64_t k, bool *has_sigma) {
  const uint32_t n = cur.n[k];
  *has_sigma = n >= 2;
  return n >= 2 ? sqrt(cur.m2[k] / ((double)n - 1.0)) : 0.0;   // k_key_sigma: sqrt(m2 / (cnt - 1.0))
}

__device__ __forceinline__ void win_row(OutRows out, unsigned long long at, uint64_t k, long long ts, double x, double e, double sg, bool all,
                                        bool verdict) {
  out.key_id[at] = k;
  out.flow_end_s[at] = ts;
  out.throughput[at] = x;
  out.algo_calc[at] = e;
  out.stddev[at] = sg;
  if (all) out.anomaly[at] = verdict ? 1 : 0;
}

// tmin: the smallest first time of a non-empty key, biased by 2^63 so that the unsigned minimum is the signed one (~0 = no point)
__global__ __launch_bounds__(kWBlock) void k_win_route(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                      unsigned long long coop_min, uint32_t *__restrict__ list, unsigned int *__restrict__ count,
                                                      unsigned long long *__restrict__ tmin) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  unsigned long long p0 = 0, len = 0;
  if (k < K) { p0 = soff[k]; len = soff[k + 1] - p0; }
  const bool is_long = len >= coop_min;
  const unsigned long long m = __ballot(is_long);
  if (m) {
    const int first = __ffsll((long long)m) - 1;
    unsigned int base = 0;
    if ((int)lane == first) base = atomicAdd(count, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, first);
    if (is_long) list[base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)k;
  }
  unsigned long long t = len ? ((unsigned long long)st[p0] ^ (1ull << 63)) : ~0ull;
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(t, d);
    t = o < t ? o : t;
  }
  if (lane == 0 && t != ~0ull) atomicMin(tmin, t);
}

template <bool EMIT, bool ALL>
__global__ __launch_bounds__(kWBlock) void k_win_ewma(uint64_t K, const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ sval,
                                                     const long long *__restrict__ st, StreamState cur, double alpha, unsigned long long coop_min,
                                                     uint32_t *__restrict__ n_anom, const unsigned long long *__restrict__ off, OutRows out,
                                                     const uint32_t *__restrict__ first) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  if (k >= K) return;
  const unsigned long long p0 = soff[k], len = soff[k + 1] - p0;
  if (len >= coop_min) return;   // k_win_ewma_coop's
  if (len == 0) {
    if (!EMIT) n_anom[k] = 0;
    return;
  }
  bool has_sigma;
  const double sg = win_sigma(cur, k, &has_sigma);
  const double one_minus = 1.0 - alpha;
  double e = 0.0;
  uint32_t a = 0;
  unsigned long long pos = EMIT ? off[k] : 0ull;
  const unsigned long long f = first ? first[k] : 0ull;   // tad_run_state_since: points before index f are walked, not counted or emitted
  const unsigned long long nch = (len + kWinChunk - 1) / kWinChunk;
  unsigned long long va[kWinChunk], vb[kWinChunk];
  long long ta[kWinChunk], tb[kWinChunk];
  // chunk c of the lane's segment; an index past the end re-reads the last point (in bounds, the load count stays fixed)
  auto load = [&](unsigned long long c, unsigned long long *v, long long *t) {
#pragma unroll
    for (int u = 0; u < kWinChunk; ++u) {
      const unsigned long long i = c * kWinChunk + u;
      const unsigned long long at = p0 + (i < len ? i : len - 1);
      v[u] = sval[at];
      if (EMIT) t[u] = st[at];
    }
  };
  auto consume = [&](unsigned long long c, const unsigned long long *v, const long long *t) {
#pragma unroll
    for (int u = 0; u < kWinChunk; ++u) {
      if (c * kWinChunk + u >= len) break;
      const double x = (double)v[u];
      e = one_minus * e + alpha * x;
      const bool verdict = has_sigma && fabs(x - e) > sg;
      if ((ALL || verdict) && c * kWinChunk + u >= f) {
        if (EMIT) win_row(out, pos++, k, t[u], x, e, sg, ALL, verdict);
        a++;
      }
    }
  };
  load(0, va, ta);
  for (unsigned long long c = 0; c < nch; c += 2) {
    load(c + 1 < nch ? c + 1 : c, vb, tb);
    consume(c, va, ta);
    load(c + 2 < nch ? c + 2 : nch - 1, va, ta);
    if (c + 1 < nch) consume(c + 1, vb, tb);
  }
  if (!EMIT) n_anom[k] = a;
}

// The emit pass for anomalous rows, staged through LDS (see the head of this file).  One workgroup = one wavefront = 64 consecutive keys.
// Rows of keys that k_win_ewma_coop owns lie inside the wavefront's range too: their places keep the "nobody parked here" mark and are
// skipped by the flush.
static constexpr uint32_t kWinNoLane = 0xFFu;
__global__ __launch_bounds__(64) void k_win_emit_staged(uint64_t K, const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ sval,
                                                        const long long *__restrict__ st, StreamState cur, double alpha, unsigned long long coop_min,
                                                        const unsigned long long *__restrict__ off, OutRows out, uint32_t cap,
                                                        const uint32_t *__restrict__ first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_win[];
  double *s_e = reinterpret_cast<double *>(smem_win);                  // [cap]
  double *s_sg = s_e + cap;                                            // [64]
  uint32_t *s_p = reinterpret_cast<uint32_t *>(s_sg + 64);             // [cap] the point, relative to the wavefront's first
  uint8_t *s_l = reinterpret_cast<uint8_t *>(s_p + cap);               // [cap] the lane that parked the row
  const uint32_t lane = threadIdx.x;
  const uint64_t k0 = (uint64_t)blockIdx.x * 64;
  const uint64_t k = k0 + lane;
  const uint64_t kend = k0 + 64 < K ? k0 + 64 : K;
  const unsigned long long base = off[k0];
  const unsigned long long total = off[kend] - base;
  if (total == 0) return;   // uniform over the wavefront
  const bool live = k < K;
  const unsigned long long pbase = soff[k0];
  const unsigned long long p0 = live ? soff[k] : 0ull;
  unsigned long long len = live ? soff[k + 1] - p0 : 0ull;
  if (len >= coop_min) len = 0;   // k_win_ewma_coop's
  unsigned long long pos = live ? off[k] - base : 0ull;
  const unsigned long long end = live ? off[k + 1] - base : 0ull;
  bool has_sigma = false;
  const double sg = len ? win_sigma(cur, k, &has_sigma) : 0.0;
  s_sg[lane] = sg;
  const uint32_t mycap = soff[kend] - pbase < (1ull << 32) ? cap : 0u;   // (the relative point index is 32 bits wide)
  const unsigned long long staged = total < mycap ? total : mycap;
  for (unsigned long long r = lane; r < staged; r += 64) s_l[r] = (uint8_t)kWinNoLane;
  __syncthreads();
  if (len != 0 && pos != end) {   // (rows imply a defined sigma: the count pass counts nothing otherwise)
    const double one_minus = 1.0 - alpha;
    double e = 0.0;
    const unsigned long long f = first ? first[k] : 0ull;
    const unsigned long long nch = (len + kWinChunk - 1) / kWinChunk;
    unsigned long long va[kWinChunk], vb[kWinChunk];
    auto load = [&](unsigned long long c, unsigned long long *v) {
#pragma unroll
      for (int u = 0; u < kWinChunk; ++u) {
        const unsigned long long i = c * kWinChunk + u;
        v[u] = sval[p0 + (i < len ? i : len - 1)];
      }
    };
    auto consume = [&](unsigned long long c, const unsigned long long *v) {
#pragma unroll
      for (int u = 0; u < kWinChunk; ++u) {
        const unsigned long long i = c * kWinChunk + u;
        if (i >= len) break;
        const double x = (double)v[u];
        e = one_minus * e + alpha * x;
        if (has_sigma && fabs(x - e) > sg && i >= f && pos < end) {
          if (pos < staged) {
            s_e[pos] = e;
            s_p[pos] = (uint32_t)(p0 + i - pbase);
            s_l[pos] = (uint8_t)lane;
          } else {
            win_row(out, base + pos, k, st[p0 + i], x, e, sg, false, true);
          }
          pos++;
        }
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
  __syncthreads();
  for (unsigned long long r = lane; r < staged; r += 64) {
    const uint32_t ln = s_l[r];
    if (ln == kWinNoLane) continue;
    const unsigned long long p = pbase + s_p[r];
    const unsigned long long at = base + r;
    out.key_id[at] = k0 + ln;
    out.flow_end_s[at] = st[p];
    out.throughput[at] = (double)sval[p];
    out.algo_calc[at] = s_e[r];
    out.stddev[at] = s_sg[ln];
  }
}

// One wavefront per listed key, grid-stride over the list.
template <bool EMIT, bool ALL>
__global__ __launch_bounds__(kWBlock) void k_win_ewma_coop(const uint32_t *__restrict__ list, const unsigned int *__restrict__ count,
                                                          const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ sval,
                                                          const long long *__restrict__ st, StreamState cur, double alpha,
                                                          uint32_t *__restrict__ n_anom, const unsigned long long *__restrict__ off, OutRows out,
                                                          const uint32_t *__restrict__ first) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = (blockIdx.x * kWBlock + threadIdx.x) >> 6, nwaves = gridDim.x * (kWBlock / 64);
  const unsigned total = *count;
  for (unsigned ent = wave; ent < total; ent += nwaves) {   // wavefront-uniform
    const uint64_t k = list[ent];
    const unsigned long long p0 = soff[k], len = soff[k + 1] - p0;
    const unsigned long long nblk = (len + 63) / 64;
    bool has_sigma;
    const double sg = win_sigma(cur, k, &has_sigma);
    const double one_minus = 1.0 - alpha;
    double e = 0.0;
    uint32_t a = 0;
    unsigned long long pos = EMIT ? off[k] : 0ull;
    const unsigned long long f = first ? first[k] : 0ull;
    auto load = [&](unsigned long long c, unsigned long long &v, long long &t) {
      const unsigned long long i = c * 64 + lane;
      const bool in = c < nblk && i < len;
      v = in ? sval[p0 + i] : 0ull;
      t = (EMIT && in) ? st[p0 + i] : 0ll;
    };
    unsigned long long v0, v1, v2;
    long long t0, t1, t2;
    load(0, v0, t0);
    load(1, v1, t1);
    for (unsigned long long c = 0; c < nblk; ++c) {
      load(c + 2, v2, t2);
      const unsigned long long left = len - c * 64;
      const int cnt = __builtin_amdgcn_readfirstlane((int)(left < 64 ? left : 64));   // points of this block (scalar)
      const double x0 = (double)v0;   // every lane converts its own point
      double my_e = 0.0;
      bool my_verdict = false;
      for (int u = 0; u < cnt; ++u) {
        const double x = readlane_f64(x0, u);
        e = one_minus * e + alpha * x;
        const bool verdict = has_sigma && fabs(x - e) > sg;
        if ((int)lane == u) { my_e = e; my_verdict = verdict; }
      }
      const unsigned long long m = __ballot((ALL ? (int)lane < cnt : my_verdict) && c * 64 + lane >= f);
      if (EMIT && ((m >> lane) & 1ull))
        win_row(out, pos + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull)), k, t0, x0, my_e, sg, ALL, my_verdict);
      pos += (unsigned long long)__popcll(m);
      a += (uint32_t)__popcll(m);
      v0 = v1; t0 = t1;
      v1 = v2; t1 = t2;
    }
    if (!EMIT && lane == 0) n_anom[k] = a;
  }
}

// One wavefront per key: nk[i] = k for the key's points, coalesced.
__global__ __launch_bounds__(kWBlock) void k_win_keys(uint64_t K, const unsigned long long *__restrict__ soff, unsigned long long *__restrict__ nk) {
  const uint64_t k = ((uint64_t)blockIdx.x * kWBlock + threadIdx.x) >> 6;   // wavefront-uniform
  if (k >= K) return;
  const unsigned long long p1 = soff[k + 1];
  for (unsigned long long i = soff[k] + (threadIdx.x & 63u); i < p1; i += 64) nk[i] = k;
}

// ---- tad_run_state_window: a transient view of every key's points inside a window (include/tad.h) ----
// The window keeps an INTERIOR range of every key's series — the points with from_t <= t < to_t, then the newest keep_points of those —
// where tad_state_trim keeps a suffix.  The view is what a state trimmed to the window would hold, built in context workspace and never
// in the state: CSR offsets woff[K + 1], values wval[] and times wt[], window moments, and for DBSCAN the window's values sorted per key.
// The kernels above and the stream's DBSCAN / ARIMA kernels then run on the view unchanged.
//   1. k_win_bounds, one lane per key: two lower-bound searches in the key's times [soff[k], soff[k + 1]) for from_t and to_t, then the
//      count rule.  Per key: the window's first point (relative to the segment), its length, the excluded count (prefix + suffix) and
//      the wavefronts of the copy (the key's OLD segment in chunks of kHistChunk: k_hist_subtract walks the history by the same chunks).
//      The scan of the lengths is woff, and woff[K] the window's point total; the excluded total is the state's points minus that.
//      Traffic: 16 B of offsets and 16 B of results per key, plus 2 x log2(len) dependent 8-byte loads.  With a key mask
//      (tad_run_state_keys / tad_drop_state_keys: keep[k], one byte per key) a key that is not selected gets an empty window with all
//      its points excluded and searches nothing; everything after this kernel treats it as a key the window left empty.
//   2. k_win_gather, one wavefront per chunk, lanes on consecutive points (coalesced 8-byte loads and stores): the interior range of
//      values and times to woff[k]; with `ev` the excluded values, prefix then suffix, packed at eoff[k].  Without `ev` a wavefront
//      touches only its part of the interior range.  Model: 32 B per window point (value and time, read and written) plus 16 B per
//      packed excluded value (read and written; the issue's model counts the write alone).
//   3. the moments: launch_trim_moments with rcnt = the window lengths, ecnt = the excluded counts, the view's series as the "new" one:
//      a cut key is replayed from the zero state with stream_step, a whole key takes the state's moments, a key left empty is unseen.
//      The replay is one lane's serial chain as long as the cut key's window, as for a trim (k_trim_moments prefetches the values).
//   4. DBSCAN's window history, one rule per call (win_hist_by_sort): sort the window's values per key (launch_hist_sort over wval /
//      woff), or sort the packed excluded values and remove them from the state's history (launch_hist_subtract).  Same bits either way:
//      both are the sorted multiset of the key's window values.
// No kernel here reads a series slot outside [soff[k], soff[k + 1]) or writes anything but the workspace arrays it is handed.
__device__ __forceinline__ unsigned long long win_lower_t(const long long *__restrict__ st, unsigned long long lo, unsigned long long hi, long long t) {
  while (lo < hi) { const unsigned long long mid = lo + ((hi - lo) >> 1); if (st[mid] < t) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ __launch_bounds__(kWBlock) void k_win_bounds(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                       long long from_t, long long to_t, uint64_t keep_points, const uint8_t *__restrict__ keep,
                                                       const long long *__restrict__ since, uint32_t *__restrict__ wbeg, uint32_t *__restrict__ wlen, uint32_t *__restrict__ ecnt,
                                                       uint32_t *__restrict__ chunks) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  if (k >= K) return;
  const unsigned long long o0 = soff[k], o1 = soff[k + 1], len = o1 - o0;
  // a key that is not selected (tad_run_state_keys' mask; tad_run_state_since: a key without a change): no window point, every point
  // excluded, no search
  if ((keep != nullptr && keep[k] == 0) || (since != nullptr && since[k] == kNoChange)) {
    wbeg[k] = 0;
    wlen[k] = 0;
    ecnt[k] = (uint32_t)len;
    chunks[k] = len > kHistChunk ? (uint32_t)((len + kHistChunk - 1) / kHistChunk) : 1u;   // (k_hist_subtract walks the history by these)
    return;
  }
  unsigned long long lo = from_t != 0 ? win_lower_t(st, o0, o1, from_t) - o0 : 0ull;          // the first point at or after from_t
  const unsigned long long hi = to_t != 0 ? win_lower_t(st, o0 + lo, o1, to_t) - o0 : len;     // the first point at or after to_t (>= lo)
  if (keep_points != 0 && hi - lo > keep_points) lo = hi - keep_points;
  wbeg[k] = (uint32_t)lo;
  wlen[k] = (uint32_t)(hi - lo);
  ecnt[k] = (uint32_t)(len - (hi - lo));
  chunks[k] = len > kHistChunk ? (uint32_t)((len + kHistChunk - 1) / kHistChunk) : 1u;   // (an empty key too: see chunk_key_min1)
}

__global__ __launch_bounds__(kWBlock) void k_win_gather(const unsigned long long *__restrict__ coff, uint64_t K, const unsigned long long *__restrict__ soff,
                                                       const unsigned long long *__restrict__ sval, const long long *__restrict__ st,
                                                       const uint32_t *__restrict__ wbeg, const unsigned long long *__restrict__ woff,
                                                       unsigned long long *__restrict__ wval, long long *__restrict__ wt,
                                                       const unsigned long long *__restrict__ eoff, unsigned long long *__restrict__ ev) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kWBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key_min1(coff, K, w);   // (coff: the scan of k_win_bounds' chunks, at least one for every key)
  const unsigned long long o0 = soff[k], len = soff[k + 1] - o0;
  const unsigned long long d0 = woff[k], n = woff[k + 1] - d0;
  const unsigned long long b = wbeg[k], be = b + n;   // the interior range [b, be) of the segment
  unsigned long long c0 = (w - coff[k]) * kHistChunk, c1 = c0 + kHistChunk;
  if (c1 > len) c1 = len;
  if (!ev) {   // only the interior part of this chunk
    if (c0 < b) c0 = b;
    if (c1 > be) c1 = be;
  }
  const unsigned long long e0 = ev ? eoff[k] : 0ull;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    const unsigned long long x = sval[o0 + u];
    if (u >= b && u < be) {
      wval[d0 + u - b] = x;
      wt[d0 + u - b] = st[o0 + u];
    } else {
      ev[e0 + (u < b ? u : u - n)] = x;   // (reached with ev only: without it the loop stays inside [b, be))
    }
  }
}

// ---- tad_run_state_since / tad_drop_state_since: judge the view, report from a time on (include/tad.h) ----
// Times ascend per key, so the reported points of a key — t >= since_t, t >= key_since[k] — are a SUFFIX of its view segment.
//   k_win_since   one lane per key: first[k] = the suffix's first index (one lower bound over the view's times for the larger of the two
//                 thresholds; the whole segment without one; len for a key whose key_since is kNoChange), cnt[k] = the suffix's length,
//                 chunks[k] = its wavefronts in k_win_suffix (0 for an empty one); n_keys (DROP, whose judged keys nothing else counts)
//                 += the keys with a view point, one atomic per wavefront.  The scan of cnt is poff.
//   k_win_suffix  one wavefront per kHistChunk points of one key's suffix, lanes on consecutive points (coalesced 8-byte loads and
//                 stores), k_win_gather's manner: key, time and value of every reported point packed at poff[k].  That is the HistBatch
//                 of "new points" the stream detectors judge against the whole view (hist_verdicts, stream_arima_batch, state_drop_batch).
// EWMA walks the series anyway: the three kernels above take first[k] and count or emit a point only at an index >= first[k].
__global__ __launch_bounds__(kWBlock) void k_win_since(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                      const long long *__restrict__ key_since, long long since_t, long long bucket_s,
                                                      long long bucket_origin, uint32_t *__restrict__ first, uint32_t *__restrict__ cnt,
                                                      uint32_t *__restrict__ chunks, unsigned long long *__restrict__ n_keys) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  unsigned long long len = 0;
  if (k < K) {
    const unsigned long long o0 = soff[k];
    len = soff[k + 1] - o0;
    bool bounded = since_t != 0, selected = true;
    long long thr = since_t;
    if (key_since != nullptr) {
      const long long ks = key_since[k];
      if (ks == kNoChange) selected = false;
      else if (!bounded || ks > thr) { thr = ks; bounded = true; }
    }
    // tad_run_state_buckets (the view's times are bucket starts): the bucket that holds the threshold is reported whole
    if (bucket_s != 0 && bounded) thr = bucket_start(thr, bucket_s, bucket_origin);
    const unsigned long long f = !selected ? len : (bounded ? win_lower_t(st, o0, o0 + len, thr) - o0 : 0ull);
    first[k] = (uint32_t)f;
    if (cnt != nullptr) {   // (NULL: the caller wants first[k] alone — EWMA's anomalous rows, counted by the walk)
      cnt[k] = (uint32_t)(len - f);
      chunks[k] = (uint32_t)((len - f + kHistChunk - 1) / kHistChunk);
    }
  }
  if (n_keys != nullptr) {   // (uniform: every lane of the wavefront reaches the ballot)
    const unsigned long long m = __ballot(len != 0);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(n_keys, (unsigned long long)__popcll(m));
  }
}

__global__ __launch_bounds__(kWBlock) void k_win_suffix(const unsigned long long *__restrict__ coff, uint64_t K, const unsigned long long *__restrict__ soff,
                                                       const unsigned long long *__restrict__ sval, const long long *__restrict__ st,
                                                       const uint32_t *__restrict__ first, const unsigned long long *__restrict__ poff,
                                                       unsigned long long *__restrict__ nk, long long *__restrict__ nt,
                                                       unsigned long long *__restrict__ nv) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kWBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key(coff, K, w);   // (wavefront-uniform; a key with an empty suffix has no chunk)
  const unsigned long long src = soff[k] + first[k], d0 = poff[k], n = poff[k + 1] - d0;
  const unsigned long long c0 = (w - coff[k]) * kHistChunk;
  unsigned long long c1 = c0 + kHistChunk;
  if (c1 > n) c1 = n;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    nk[d0 + u] = k;
    nt[d0 + u] = st[src + u];
    nv[d0 + u] = sval[src + u];
  }
}

// ---- tad_run_state_buckets: the window's points folded into time buckets, straight from the state's arrays (include/tad.h) ----
// Times ascend per key, so a bucket — the points of one key with the same bucket_start (tad_bucket.h) — is a contiguous RUN of the key's
// window range [beg, beg + len) of its segment: a segmented fold and a compaction, no sort, no hash, no K x T grid.  A HEAD is a point
// whose bucket differs from its predecessor's in the key; the key's first window point always is one.  The chunks are k_win_gather's
// (coff from k_win_bounds: kHistChunk consecutive points of one key's segment per wavefront, lanes on consecutive points), ordered by key
// and then position, so the scan of the chunks' head counts is every chunk's first destination cell, and the cell before it is the one
// of the run open at the chunk's first point.
//   k_win_bucket_heads  per chunk: the heads inside the key's window range (ballot + popcount per 64-point slice);
//   k_win_bucket_fold   the same chunks, per slice: bucket start, head flag (lane 0 against the element before the slice), rank by ballot
//                       and popcount, a segmented inclusive scan of the values across the wavefront (six shuffle steps, unsigned 64-bit,
//                       wrapping add or unsigned maximum), the run left open at lane 63 carried in registers into the next slice.  A run
//                       whose head and end both lie in the chunk takes ONE plain store; a partial of a run that crosses a chunk edge (it
//                       may span several chunks) is one 64-bit atomicAdd / atomicMax onto its cell, zeroed beforehand — an integer
//                       operation, so the result does not depend on the order.  The head's owner writes the bucket start.  No LDS, no
//                       scratch, no floating point;
//   k_win_bucket_keys   one lane per key: the view's offsets boff[k] = the destination of the key's first chunk, the buckets per key and
//                       the points folded away or cut (what launch_trim_moments takes as rcnt / ecnt).
// The source is described by offsets and ranges and the destination by plain arrays (BucketSource): tad_state_rollup (tad_capi_state.cpp)
// runs the same two kernels with ROLLUP = true over every key's whole segment, its destination the state's candidate arenas.  No kernel here reads a series slot outside the key's range or writes a cell >= buckets.
// The bucket function of a launch, passed by value: the two numbers of tad_run_state_buckets (two 8-byte kernel arguments, as before the
// roll-up existed), and for tad_state_rollup the bound as well — rollup_start (tad_bucket.h): a point at or after the bound is a bucket of
// its own.
template <bool ROLLUP> struct BucketFn;
template <> struct BucketFn<false> {
  long long bucket_s, origin;
  __device__ __forceinline__ long long operator()(long long t) const { return bucket_start(t, bucket_s, origin); }
};
template <> struct BucketFn<true> {
  long long bucket_s, origin, bound;
  __device__ __forceinline__ long long operator()(long long t) const { return rollup_start(t, bound, bucket_s, origin); }
};

template <bool ROLLUP>
__device__ __forceinline__ bool bucket_head(const long long *__restrict__ st_key, unsigned long long u, bool valid, unsigned long long beg, unsigned lane,
                                            const BucketFn<ROLLUP> &fn, long long *start) {
  const long long s = valid ? fn(st_key[u]) : 0ll;
  long long prev = __shfl_up(s, 1);
  if (lane == 0 && valid && u > beg) prev = fn(st_key[u - 1]);   // the element before the slice
  *start = s;
  return valid && (u == beg || s != prev);
}

// the part [c0, c1) of chunk w's points that lies inside its key's range; false: none
__device__ __forceinline__ bool bucket_chunk(const unsigned long long *__restrict__ coff, uint64_t K, const BucketSource &src, unsigned long long w, uint64_t *key,
                                             unsigned long long *o0, unsigned long long *beg, unsigned long long *end, unsigned long long *c0,
                                             unsigned long long *c1) {
  const uint64_t k = chunk_key_min1(coff, K, w);
  const unsigned long long len = src.soff[k + 1] - src.soff[k];
  const unsigned long long b = src.beg[k], be = b + src.len[k];
  unsigned long long a0 = (w - coff[k]) * kHistChunk, a1 = a0 + kHistChunk;
  if (a1 > len) a1 = len;
  if (a0 < b) a0 = b;
  if (a1 > be) a1 = be;
  *key = k; *o0 = src.soff[k]; *beg = b; *end = be; *c0 = a0; *c1 = a1;
  return a0 < a1;
}

// ROLLUP (tad_state_rollup): a chunk whose first point is at or after the bound holds only buckets of one point — times ascend, and its
// first point is a head because its predecessor's image lies below the bound — so its heads are its points and it reads one time.
template <bool ROLLUP>
__global__ __launch_bounds__(kWBlock) void k_win_bucket_heads(const unsigned long long *__restrict__ coff, uint64_t K, uint64_t chunks_bound, BucketSource src,
                                                             BucketFn<ROLLUP> fn, uint32_t *__restrict__ hcnt) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kWBlock + threadIdx.x) >> 6;
  if (w >= chunks_bound) return;
  const unsigned lane = threadIdx.x & 63u;
  uint32_t heads = 0;
  if (w < coff[K]) {   // (wavefront-uniform; the entries past the last chunk are scanned too and must be 0)
    uint64_t k;
    unsigned long long o0, beg, end, c0, c1;
    if (bucket_chunk(coff, K, src, w, &k, &o0, &beg, &end, &c0, &c1)) {
      bool tail = false;   // (wavefront-uniform: every lane reads the same time)
      if constexpr (ROLLUP) tail = src.st[o0 + c0] >= fn.bound;
      if (tail) heads = (uint32_t)(c1 - c0);
      else
        for (unsigned long long u0 = c0; u0 < c1; u0 += 64) {
          const unsigned long long u = u0 + lane;
          long long start;
          const bool head = bucket_head(src.st + o0, u, u < c1, beg, lane, fn, &start);
          heads += (uint32_t)__popcll(__ballot(head));
        }
    }
  }
  if (lane == 0) hcnt[w] = heads;
}

template <bool MAX> __device__ __forceinline__ unsigned long long bucket_op(unsigned long long a, unsigned long long b) {
  return MAX ? (a > b ? a : b) : a + b;
}

// ROLLUP: a chunk wholly at or after the bound (k_win_bucket_heads' test) is a copy — coalesced loads and stores of values and times to
// hoff[w] + (u - c0), no shuffle, no atomic.  The chunk that holds the split and the chunks below it take the fold; the points of the
// split chunk at or after the bound are runs of one there.
template <bool MAX, bool ROLLUP>
__global__ __launch_bounds__(kWBlock) void k_win_bucket_fold(const unsigned long long *__restrict__ coff, uint64_t K, BucketSource src, BucketFn<ROLLUP> fn,
                                                            const unsigned long long *__restrict__ hoff, uint64_t buckets,
                                                            unsigned long long *__restrict__ bval, long long *__restrict__ bt) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kWBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  uint64_t k;
  unsigned long long o0, beg, end, c0, c1;
  if (!bucket_chunk(coff, K, src, w, &k, &o0, &beg, &end, &c0, &c1)) return;
  // the chunk's first head goes to cell hoff[w]; the run open at its first point (head in an earlier chunk of the key) is the cell before
  unsigned long long cell_next = hoff[w];
  if constexpr (ROLLUP) {
    if (src.st[o0 + c0] >= fn.bound) {   // (wavefront-uniform)
      for (unsigned long long u = c0 + lane; u < c1; u += 64) {
        const unsigned long long cell = cell_next + (u - c0);
        if (cell < buckets) { bval[cell] = src.sval[o0 + u]; bt[cell] = src.st[o0 + u]; }
      }
      return;
    }
  }
  // the run open at a slice's first point: what this chunk has folded of it so far, and whether its head lies in this chunk
  unsigned long long carry = 0;
  bool carry_head = false;
  for (unsigned long long u0 = c0; u0 < c1; u0 += 64) {   // (wavefront-uniform)
    const unsigned long long u = u0 + lane;
    const bool valid = u < c1;
    long long start;
    const bool head = bucket_head(src.st + o0, u, valid, beg, lane, fn, &start);
    unsigned long long x = valid ? src.sval[o0 + u] : 0ull;
    const unsigned long long hm = __ballot(head);
    // the run carried out of the previous slice ended at its lane 63: this slice opens with a head
    if (lane == 0 && head && u0 != c0 && cell_next - 1 < buckets) {
      if (carry_head) bval[cell_next - 1] = carry;
      else if (MAX) atomicMax(bval + cell_next - 1, carry);
      else atomicAdd(bval + cell_next - 1, carry);
    }
    // segmented inclusive scan: after it x folds the lane's run from its head (or from lane 0) up to the lane
    bool seen = head;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
      const unsigned long long xo = __shfl_up(x, d);
      const int so = __shfl_up((int)seen, d);
      if (lane >= d && !seen) { x = bucket_op<MAX>(xo, x); seen = so != 0; }
    }
    const unsigned r = (unsigned)__popcll(hm & (~0ull >> (63u - lane)));   // heads at or before this lane
    if (r == 0) x = bucket_op<MAX>(carry, x);
    const bool head_here = r != 0 || carry_head;      // the run's head lies in this chunk
    const unsigned long long cell = cell_next + r - 1;
    const bool next_valid = u + 1 < c1;
    const bool next_head = lane < 63u && ((hm >> (lane + 1u)) & 1ull) != 0;
    if (head && cell < buckets) bt[cell] = start;
    if (valid && (next_head || !next_valid) && cell < buckets) {   // the run ends here: at a head, at the range's end, or at the chunk's edge
      if (head_here && (next_head || c1 == end)) bval[cell] = x;   // whole inside the chunk: nobody else writes the cell
      else if (MAX) atomicMax(bval + cell, x);
      else atomicAdd(bval + cell, x);
    }
    // (lane 63 with a valid successor: the run is still open — carried; whether it ends there the next slice's lane 0 finds out)
    carry = __shfl(x, 63);
    carry_head = __shfl((int)head_here, 63) != 0;
    cell_next += (unsigned long long)__popcll(hm);
  }
}

__global__ __launch_bounds__(kWBlock) void k_win_bucket_keys(uint64_t K, const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ coff,
                                                            const unsigned long long *__restrict__ hoff, unsigned long long *__restrict__ boff,
                                                            uint32_t *__restrict__ bcnt, uint32_t *__restrict__ becnt) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  if (k > K) return;
  const unsigned long long b0 = hoff[coff[k]];
  boff[k] = b0;
  if (k == K) return;
  const unsigned long long nb = hoff[coff[k + 1]] - b0;
  bcnt[k] = (uint32_t)nb;
  becnt[k] = (uint32_t)(soff[k + 1] - soff[k] - nb);
}

// tad_state_rollup, k_win_bucket_keys' place: the candidate series offsets, per key the points afterwards and the points folded away (what
// launch_trim_moments takes as rcnt / ecnt), and the call's counters.  A key's points below the bound: one lower bound over its OLD times;
// all of its folded points lie among them.  One atomic per wavefront and counter.
__global__ __launch_bounds__(kWBlock) void k_rollup_keys(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                        const unsigned long long *__restrict__ coff, const unsigned long long *__restrict__ hoff,
                                                        long long bound, unsigned long long *__restrict__ boff, uint32_t *__restrict__ rcnt,
                                                        uint32_t *__restrict__ ecnt, RollupCounters *__restrict__ rc) {
  const uint64_t k = (uint64_t)blockIdx.x * kWBlock + threadIdx.x;
  unsigned long long below = 0, folded = 0;
  if (k <= K) {
    const unsigned long long b0 = hoff[coff[k]];
    boff[k] = b0;
    if (k < K) {
      const unsigned long long o0 = soff[k], o1 = soff[k + 1];
      const unsigned long long nb = hoff[coff[k + 1]] - b0;
      folded = o1 - o0 - nb;
      rcnt[k] = (uint32_t)nb;
      ecnt[k] = (uint32_t)folded;
      below = win_lower_t(st, o0, o1, bound) - o0;
    }
  }
  unsigned long long after = below - folded;   // the points the key holds below the bound afterwards
  const unsigned long long changed = __ballot(folded != 0);
#pragma unroll
  for (unsigned d = 32; d >= 1; d >>= 1) {   // (every lane of the wavefront is here)
    below += __shfl_down(below, d);
    after += __shfl_down(after, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (below) atomicAdd(&rc->rolled, below);
    if (after) atomicAdd(&rc->buckets, after);
    if (changed) atomicAdd(&rc->keys_changed, (unsigned long long)__popcll(changed));
  }
}

// ---- launchers ----
static inline unsigned win_blocks(uint64_t lanes) { return (unsigned)((lanes + kWBlock - 1) / kWBlock); }

// A key takes a wavefront of its own when it is long (>= kCoopMinT points, the grid's rule) and a lane would be the tail of the launch:
// either there are few keys anyway (<= kCoopMaxK: the chip is not full of lanes) or the key is eight times the average length.  A
// wavefront per key costs 64 lanes of arithmetic for one key's recurrence, so a window of many equally long keys stays on lanes.
unsigned long long win_coop_min(uint64_t K, uint64_t points) {
  if (K <= kCoopMaxK) return kCoopMinT;
  const unsigned long long outlier = 8 * (points / K + 1);
  return outlier > kCoopMinT ? outlier : kCoopMinT;
}

void launch_win_route(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, unsigned long long coop_min, uint32_t *list,
                      unsigned int *count, unsigned long long *tmin) {
  hipMemsetAsync(count, 0, sizeof(unsigned int), s);
  hipMemsetAsync(tmin, 0xFF, sizeof(unsigned long long), s);
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_route, dim3(win_blocks(K)), dim3(kWBlock), 0, s, K, soff, st, coop_min, list, count, tmin);
}

// LDS rows per wavefront of the staged emit (emit_stage_rows' rule in tad_kernels.hip): the mean row count of a 64-key range plus 1/8
// plus 128 rows, at most 4096 (52 KB: three wavefronts a CU).  tad_plan: ewma_emit = 1 -> k_win_ewma writes the rows itself;
// ewma_emit_rows pins the capacity (tests).
static uint32_t win_stage_rows(uint64_t K, uint64_t rows, int ewma_emit, uint32_t ewma_emit_rows) {
  if (ewma_emit == 1) return 0;
  const uint64_t mean = (rows * 64 + K - 1) / K;
  uint64_t cap = mean + mean / 8 + 128;
  if (ewma_emit_rows != 0) cap = ewma_emit_rows;
  cap = (cap + 63) & ~63ull;
  if (cap < 64) cap = 64;
  if (cap > 4096) cap = 4096;
  return (uint32_t)cap;
}

void launch_win_ewma(hipStream_t s, uint64_t K, const unsigned long long *soff, const unsigned long long *sval, const long long *st, StreamState cur,
                     double alpha, unsigned long long coop_min, const uint32_t *list, const unsigned int *count, bool emit, bool all_points,
                     uint32_t *n_anom, const unsigned long long *off, OutRows out, uint64_t rows, int ewma_emit, uint32_t ewma_emit_rows,
                     const uint32_t *first) {
  if (K == 0) return;
  const unsigned cwaves = (unsigned)(K < 8192 ? K : 8192);   // wavefronts that stride over the list of long keys
#define TAD_WIN_COOP(E, A)                                                                                                                     \
  hipLaunchKernelGGL((k_win_ewma_coop<E, A>), dim3(win_blocks((uint64_t)cwaves * 64)), dim3(kWBlock), 0, s, list, count, soff, sval, st, cur, \
                     alpha, n_anom, off, out, first)
#define TAD_WIN(E, A)                                                                                                                              \
  do {                                                                                                                                             \
    hipLaunchKernelGGL((k_win_ewma<E, A>), dim3(win_blocks(K)), dim3(kWBlock), 0, s, K, soff, sval, st, cur, alpha, coop_min, n_anom, off, out, first); \
    TAD_WIN_COOP(E, A);                                                                                                                            \
  } while (0)
  if (!emit) TAD_WIN(false, false);
  else if (all_points) TAD_WIN(true, true);
  else if (const uint32_t cap = win_stage_rows(K, rows, ewma_emit, ewma_emit_rows)) {
    hipLaunchKernelGGL(k_win_emit_staged, dim3((unsigned)((K + 63) / 64)), dim3(64), (size_t)cap * 13 + 64 * 8, s, K, soff, sval, st, cur, alpha, coop_min,
                       off, out, cap, first);
    TAD_WIN_COOP(true, false);
  } else TAD_WIN(true, false);
#undef TAD_WIN
#undef TAD_WIN_COOP
}

void launch_win_keys(hipStream_t s, uint64_t K, const unsigned long long *soff, unsigned long long *nk) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_keys, dim3(win_blocks(K * 64)), dim3(kWBlock), 0, s, K, soff, nk);
}

// TAD_WIN_HIST_FORCE (measurement builds of tools/build_variants.py only; the product's build() never defines it): 1 = always sort the
// window, 2 = always subtract
bool win_hist_by_sort(uint64_t window_points, uint64_t state_points) {
#if defined(TAD_WIN_HIST_FORCE)
  return TAD_WIN_HIST_FORCE == 1;
#else
  return 2 * window_points <= state_points;
#endif
}

void launch_win_bounds(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, long long from_t, long long to_t,
                       uint64_t keep_points, const uint8_t *keep, uint32_t *wbeg, uint32_t *wlen, uint32_t *ecnt, uint32_t *chunks, const long long *since) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_bounds, dim3(win_blocks(K)), dim3(kWBlock), 0, s, K, soff, st, from_t, to_t, keep_points, keep, since, wbeg, wlen, ecnt, chunks);
}

void launch_win_since(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, const long long *key_since, long long since_t,
                      const SinceKeys &sk, bool lengths, unsigned long long *n_keys, long long bucket_s, long long bucket_origin) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_since, dim3(win_blocks(K)), dim3(kWBlock), 0, s, K, soff, st, key_since, since_t, bucket_s, bucket_origin, sk.first,
                     lengths ? sk.cnt : nullptr, lengths ? sk.chunks : nullptr, n_keys);
}

void launch_win_bucket_heads(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const BucketSource &src, long long bucket_s,
                             long long bucket_origin, uint32_t *hcnt) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_bucket_heads<false>, dim3(win_blocks(chunks_bound * 64)), dim3(kWBlock), 0, s, coff, K, chunks_bound, src,
                     BucketFn<false>{bucket_s, bucket_origin}, hcnt);
}

void launch_win_bucket_fold(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const BucketSource &src, long long bucket_s,
                            long long bucket_origin, bool op_max, const unsigned long long *hoff, uint64_t buckets, unsigned long long *bval, long long *bt) {
  if (K == 0 || buckets == 0) return;
  hipMemsetAsync(bval, 0, (size_t)buckets * 8, s);   // 0 is the identity of both operations: a chunk-edge partial is an atomic onto its cell
  const dim3 grid(win_blocks(chunks_bound * 64)), block(kWBlock);
  const BucketFn<false> fn{bucket_s, bucket_origin};
  if (op_max) hipLaunchKernelGGL((k_win_bucket_fold<true, false>), grid, block, 0, s, coff, K, src, fn, hoff, buckets, bval, bt);
  else hipLaunchKernelGGL((k_win_bucket_fold<false, false>), grid, block, 0, s, coff, K, src, fn, hoff, buckets, bval, bt);
}

void launch_rollup_heads(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const BucketSource &src, long long bound,
                         long long bucket_s, long long bucket_origin, uint32_t *hcnt) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_bucket_heads<true>, dim3(win_blocks(chunks_bound * 64)), dim3(kWBlock), 0, s, coff, K, chunks_bound, src,
                     BucketFn<true>{bucket_s, bucket_origin, bound}, hcnt);
}

void launch_rollup_fold(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const BucketSource &src, long long bound,
                        long long bucket_s, long long bucket_origin, bool op_max, const unsigned long long *hoff, uint64_t points,
                        unsigned long long *sval_new, long long *st_new) {
  if (K == 0 || points == 0) return;
  // 0 is the identity of both operations.  Only the cells of runs that cross a chunk edge receive an atomic, but which those are is known
  // to the fold alone: the whole candidate is zeroed (8 B per point afterwards; DESIGN.md §5 has the cost)
  hipMemsetAsync(sval_new, 0, (size_t)points * 8, s);
  const dim3 grid(win_blocks(chunks_bound * 64)), block(kWBlock);
  const BucketFn<true> fn{bucket_s, bucket_origin, bound};
  if (op_max) hipLaunchKernelGGL((k_win_bucket_fold<true, true>), grid, block, 0, s, coff, K, src, fn, hoff, points, sval_new, st_new);
  else hipLaunchKernelGGL((k_win_bucket_fold<false, true>), grid, block, 0, s, coff, K, src, fn, hoff, points, sval_new, st_new);
}

void launch_rollup_keys(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, const unsigned long long *coff,
                        const unsigned long long *hoff, long long bound, unsigned long long *soff_new, uint32_t *rcnt, uint32_t *ecnt, RollupCounters *rc) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_rollup_keys, dim3(win_blocks(K + 1)), dim3(kWBlock), 0, s, K, soff, st, coff, hoff, bound, soff_new, rcnt, ecnt, rc);
}

void launch_win_bucket_keys(hipStream_t s, uint64_t K, const unsigned long long *soff, const unsigned long long *coff, const unsigned long long *hoff,
                            unsigned long long *boff, uint32_t *bcnt, uint32_t *becnt) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_bucket_keys, dim3(win_blocks(K + 1)), dim3(kWBlock), 0, s, K, soff, coff, hoff, boff, bcnt, becnt);
}

uint64_t win_suffix_chunks_bound(uint64_t K, uint64_t points) { return K + points / kHistChunk + 1; }

void launch_win_suffix(hipStream_t s, uint64_t K, uint64_t points, const unsigned long long *soff, const unsigned long long *sval, const long long *st,
                       const SinceKeys &sk, const SincePts &sp) {
  if (K == 0 || points == 0) return;
  hipLaunchKernelGGL(k_win_suffix, dim3(win_blocks(win_suffix_chunks_bound(K, points) * 64)), dim3(kWBlock), 0, s, sk.coff, K, soff, sval, st, sk.first,
                     sk.poff, sp.nk, sp.nt, sp.nv);
}

void launch_win_gather(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const unsigned long long *soff,
                       const unsigned long long *sval, const long long *st, const uint32_t *wbeg, const unsigned long long *woff,
                       unsigned long long *wval, long long *wt, const unsigned long long *eoff, unsigned long long *ev) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_win_gather, dim3(win_blocks(chunks_bound * 64)), dim3(kWBlock), 0, s, coff, K, soff, sval, st, wbeg, woff, wval, wt, eoff, ev);
}

const void *code_anchor_window() { return reinterpret_cast<const void *>(&k_win_route); }

}  // namespace tad
