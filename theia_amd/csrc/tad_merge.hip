// tad_merge.hip — a batch placed BY TIME into a streaming state that keeps its series with times (include/tad.h: tad_state_merge and
// tad_state_replace).
//
// tad_run_stream appends: a row not newer than its key's last point fails the batch.  A merge takes the same batch — Stage 0's points in
// (key, time) order, nk / nt / nv with poff[K + 1], as a history batch has them (tad_history.hip) — and puts every point where its time
// says, into the candidate copies of the state.  A point at a time its key already holds meets the held value by the call's RULE:
// tad_state_merge combines them (sum or max: a re-read of the same rows under sum doubles them), tad_state_replace makes the batch the
// truth (the batch's value).  A replace may also carry a RANGE R = [from, to): every old point of EVERY key inside R that the batch does
// not name is erased.  A merge is a replace without a range and with a combining rule; the steps, and what a range adds to each:
//   1. k_merge_classify, one lane per batch point: too old (before keep_from), appended (newer than everything the key holds), combined
//      (a time the key already holds: found by a lower_bound in the key's old times; "replaced" under the replace rule) or inserted (a
//      new time in between); rank = the old points of the key before it.  Three flag arrays for the scans, the call's counters with one
//      atomic per wavefront.  A range adds nothing.
//   2. scans over the points (launch_scan): nhoff = the points that add an element (inserted / appended), aoff = the kept points (what the
//      history gains), roff = the combined points (what the history loses).
//      + range: k_merge_range, one lane per key: the erased run [e0, e1) of the key's old segment — two lower_bounds in its times — and
//        ecnt = (e1 - e0) - the combined points of the key inside the run (two lower_bounds in its batch segment, a difference of roff);
//        eoff = the scan of ecnt, whose total the host reads before anything is written.
//   3. k_merge_keys, one lane per k <= K: the per-key candidate series offsets soff_new = soff_old + nhoff[p0], the packed per-key offsets
//      of the history's gains (aoff[p0]) and losses (roff[p0]), the chunk counts of 4 and 5, replay = the key has an inserted or combined
//      point.
//      + range: soff_new loses eoff and the losses start at roff[p0] + eoff (the erased values follow the key's combined ones); an erased
//        point makes the key replay; the keys that lose every point are counted (keys_emptied).
//   4. k_merge_series, a wavefront per kMergeChunk elements of a key's [old segment | batch points] as k_hist_merge: old element u goes to
//      u + #{batch points of the key before its time that add an element}, its value rule(old, new) where a batch point hit it; a batch
//      point that adds an element goes to rank + its index among those.  Values and times are written together; a key without batch points
//      is a coalesced copy.  History states: the same lanes pack the values the history loses (old values of combined points) and gains.
//      + range: an old element inside the run that no batch point hits is dropped (its value to the history's losses, behind the key's
//        combined ones, in time order); every other element and every added batch point moves down by the erased points before it.
//   5. the history: both packed lists sorted per key (launch_hist_sort), launch_hist_subtract into a scratch arena, launch_hist_merge into
//      the candidate (tad_history.hip; the host skips the subtract when the history loses nothing).  A range adds nothing.
//   6. k_merge_moments, one lane per key: a key with replay set is replayed from the zero state over its merged series (stream_step: the
//      fresh state's bits — an emptied key holds an unseen key's), a key that only gained newer points continues from its stored state,
//      the rest is copied.  A range adds nothing.
// The change report (tad.h: tad_changes; the REPORT forms, run only by a call that asked for one): k_merge_series knows every element it
// adds, erases or gives another value; the smallest such time of a chunk lowers the key's entry of `since` with one atomic per wavefront,
// and the counters take one atomic per wavefront and counter, as count_wave's.  The append path writes no series here: a lane per key
// takes the key's first batch time (k_merge_report_keys, which on either path counts the changed keys and reduces the smallest time).
// No LDS, no scratch.  Times inside one key's batch segment ascend strictly (Stage 0 made the points unique), as the key's old times do.
#include <stdint.h>

#include "tad_internal.h"

namespace tad {

static constexpr int kMBlock = 256;
static constexpr uint32_t kMergeChunk = 2048;   // k_merge_series: elements per wavefront (32 per lane), as k_hist_merge
static_assert(kMergeChunk == kHistChunk, "the series and the history are walked by the same chunks");

// the classes of a batch point against its key's old times (a replace reads MG_COMBINED as "replaced")
enum : uint8_t { MG_NONE = 0, MG_TOO_OLD = 1, MG_APPENDED = 2, MG_INSERTED = 3, MG_COMBINED = 4 };

// first index in the ascending a[lo, hi) whose time is >= t
__device__ __forceinline__ unsigned long long lower_time(const long long *a, unsigned long long lo, unsigned long long hi, long long t) {
  while (lo < hi) { const unsigned long long mid = lo + ((hi - lo) >> 1); if (a[mid] < t) lo = mid + 1; else hi = mid; }
  return lo;
}

__device__ __forceinline__ void count_wave(bool pred, unsigned lane, unsigned long long *dst) {
  const unsigned long long m = __ballot(pred);
  if (lane == 0 && m) atomicAdd(dst, (unsigned long long)__popcll(m));
}

// ---- 1. classify ----
// Lanes in [*P_dev, P_cap) write zero flags, so that the scans may run over the host's bound P_cap.
__global__ __launch_bounds__(kMBlock) void k_merge_classify(const unsigned long long *__restrict__ nk, const long long *__restrict__ nt,
                                                           const unsigned long long *__restrict__ P_dev, uint64_t P_cap, uint64_t K,
                                                           const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                           long long keep_from, uint8_t *__restrict__ cls, uint32_t *__restrict__ rank,
                                                           uint32_t *__restrict__ f_nh, uint32_t *__restrict__ f_kept, uint32_t *__restrict__ f_hit,
                                                           MergeCounters *__restrict__ mc) {
  const uint64_t i = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  uint8_t c = MG_NONE;
  uint32_t r = 0;
  if (i < P_cap && i < *P_dev) {
    const uint64_t k = nk[i];
    if (k < K) {
      const long long t = nt[i];
      if (keep_from != 0 && t < keep_from) c = MG_TOO_OLD;
      else {
        const unsigned long long o0 = soff[k], a = soff[k + 1] - o0;
        if (a == 0 || st[o0 + a - 1] < t) { c = MG_APPENDED; r = (uint32_t)a; }   // newer than the key's last point: no search
        else {
          const unsigned long long lo = lower_time(st, o0, o0 + a, t);             // (lo < o0 + a: the last time is >= t)
          c = st[lo] == t ? MG_COMBINED : MG_INSERTED;
          r = (uint32_t)(lo - o0);
        }
      }
    }
  }
  if (i < P_cap) {
    cls[i] = c;
    rank[i] = r;
    f_nh[i] = (c == MG_APPENDED || c == MG_INSERTED) ? 1u : 0u;
    f_kept[i] = c >= MG_APPENDED ? 1u : 0u;
    f_hit[i] = c == MG_COMBINED ? 1u : 0u;
  }
  count_wave(c == MG_TOO_OLD, lane, &mc->too_old);
  count_wave(c == MG_APPENDED, lane, &mc->appended);
  count_wave(c == MG_INSERTED, lane, &mc->inserted);
  count_wave(c == MG_COMBINED, lane, &mc->combined);
}

// ---- 2 + range. per key: the erased run and what it loses ----
// from / to == 0: no bound on that side.  A combined point's time is an old time, so the combined points with rank in [e0, e1) are the
// combined batch points with time in [from, to): roff[jt] - roff[jf].
__global__ __launch_bounds__(kMBlock) void k_merge_range(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                        const unsigned long long *__restrict__ poff, const long long *__restrict__ nt,
                                                        const unsigned long long *__restrict__ roff, long long from, long long to,
                                                        uint32_t *__restrict__ ebeg, uint32_t *__restrict__ eend, uint32_t *__restrict__ ecnt) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  if (k >= K) return;
  const unsigned long long o0 = soff[k], a = soff[k + 1] - o0;
  const unsigned long long e0 = from != 0 ? lower_time(st, o0, o0 + a, from) - o0 : 0ull;
  unsigned long long e1 = to != 0 ? lower_time(st, o0, o0 + a, to) - o0 : a;
  if (e1 < e0) e1 = e0;
  unsigned long long hits = 0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  if (b != 0 && e1 > e0) {
    const unsigned long long jf = from != 0 ? lower_time(nt, p0, p0 + b, from) : p0;
    const unsigned long long jt = to != 0 ? lower_time(nt, p0, p0 + b, to) : p0 + b;
    hits = jt > jf ? roff[jt] - roff[jf] : 0ull;
  }
  ebeg[k] = (uint32_t)e0;
  eend[k] = (uint32_t)e1;
  ecnt[k] = (uint32_t)((e1 - e0) - hits);
}

// ---- 3. per key: candidate offsets, packed history offsets, chunk counts, who replays ----
// One lane per k <= K.  The kept points of a key are a suffix of its batch segment (the too-old ones come first in time), and a key whose
// first kept point is newer than its last old point has only such points: replay[k] = the first kept point is inserted or combined, or
// (RANGED) the key lost a point to the range.  Only the RANGED form reads ecnt / eoff and counts into mc.
template <bool RANGED>
__global__ __launch_bounds__(kMBlock) void k_merge_keys(uint64_t K, const unsigned long long *__restrict__ poff, const unsigned long long *__restrict__ nhoff,
                                                       const unsigned long long *__restrict__ aoff, const unsigned long long *__restrict__ roff,
                                                       const uint8_t *__restrict__ cls, const unsigned long long *__restrict__ soff_old,
                                                       const unsigned long long *__restrict__ hoff_old, unsigned long long *__restrict__ soff_new,
                                                       unsigned long long *__restrict__ akoff, unsigned long long *__restrict__ rkoff,
                                                       unsigned long long *__restrict__ hoff_mid, uint32_t *__restrict__ chunks_s,
                                                       uint32_t *__restrict__ chunks_h, uint32_t *__restrict__ replay, const uint32_t *__restrict__ ecnt,
                                                       const unsigned long long *__restrict__ eoff, MergeCounters *__restrict__ mc) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  if (!RANGED && k > K) return;   // (the ranged form's lanes all reach the ballot)
  bool emptied = false;
  if (k <= K) {
    const unsigned long long p0 = poff[k];
    unsigned long long eo = 0;
    if constexpr (RANGED) eo = eoff[k];
    soff_new[k] = soff_old[k] - eo + nhoff[p0];
    if (hoff_old) {
      akoff[k] = aoff[p0];
      rkoff[k] = roff[p0] + eo;
      hoff_mid[k] = hoff_old[k] - (roff[p0] + eo);
    }
  }
  if (k < K) {
    const unsigned long long p0 = poff[k], p1 = poff[k + 1];
    const unsigned long long a = soff_old[k + 1] - soff_old[k];
    const unsigned long long len = a + (p1 - p0);
    chunks_s[k] = (uint32_t)((len + kMergeChunk - 1) / kMergeChunk);
    if (hoff_old) chunks_h[k] = (uint32_t)((hoff_old[k + 1] - hoff_old[k] + kHistChunk - 1) / kHistChunk);   // (the history kernels walk these)
    const unsigned long long kept = aoff[p1] - aoff[p0];
    bool rp = kept != 0 && cls[p1 - kept] != MG_APPENDED;
    if constexpr (RANGED) {
      const uint32_t ec = ecnt[k];
      rp = rp || ec != 0;
      emptied = a != 0 && a + (nhoff[p1] - nhoff[p0]) == (unsigned long long)ec;
    }
    replay[k] = rp ? 1u : 0u;
  }
  if constexpr (RANGED) count_wave(emptied, threadIdx.x & 63u, &mc->keys_emptied);
}

// ---- 4. the series and its times merged by time ----
// what a batch point's value y makes of the value x its key holds at that time
enum : int { MERGE_SUM = 0, MERGE_MAX = 1, MERGE_REPLACE = 2 };
template <int RULE>
__device__ __forceinline__ unsigned long long merge_value(unsigned long long x, unsigned long long y) {
  if constexpr (RULE == MERGE_SUM) return x + y;
  else if constexpr (RULE == MERGE_MAX) return x > y ? x : y;
  else return y;
}

// A key's losses in the packed list hrem start at rkoff[k]: the old values of its combined points first (point j's at its index among
// them, roff[j] - roff[p0]), then (RANGED) its erased points in time order.
// REPORT: since[k] = min(since[k], the smallest time of the chunk's changed elements) — an added batch point, an erased old point, an
// old point whose value the rule changes (a sum of 0, a maximum not above and a replace by the held value change nothing) — and
// cc->points / cc->max_t over them.
template <int RULE, bool RANGED, bool REPORT>
__global__ __launch_bounds__(kMBlock) void k_merge_series(const unsigned long long *__restrict__ coff, uint64_t K,
                                                         const unsigned long long *__restrict__ soff_old, const unsigned long long *__restrict__ sval_old,
                                                         const long long *__restrict__ st_old, const unsigned long long *__restrict__ poff,
                                                         const long long *__restrict__ nt, const unsigned long long *__restrict__ nv,
                                                         const uint8_t *__restrict__ cls, const uint32_t *__restrict__ rank,
                                                         const unsigned long long *__restrict__ nhoff, const unsigned long long *__restrict__ aoff,
                                                         const unsigned long long *__restrict__ roff, const unsigned long long *__restrict__ soff_new,
                                                         unsigned long long *__restrict__ sval_new, long long *__restrict__ st_new,
                                                         unsigned long long *__restrict__ hadd, unsigned long long *__restrict__ hrem,
                                                         const unsigned long long *__restrict__ rkoff, const uint32_t *__restrict__ ebeg,
                                                         const uint32_t *__restrict__ eend, const uint32_t *__restrict__ ecnt, long long from,
                                                         long long *__restrict__ since, ChangeCounters *__restrict__ cc) {
  static_assert(!RANGED || RULE == MERGE_REPLACE, "only a replace carries a range");
  const unsigned long long w = ((uint64_t)blockIdx.x * kMBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key(coff, K, w);   // (wavefront-uniform; a key without elements has no chunk)
  const unsigned long long o0 = soff_old[k], a = soff_old[k + 1] - o0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  const unsigned long long d0 = soff_new[k];
  const unsigned long long nh0 = b ? nhoff[p0] : 0ull;
  [[maybe_unused]] unsigned long long e0 = 0, e1 = 0, ec = 0, rf = 0, l0 = 0, nrep = 0;
  if constexpr (RANGED) {
    e0 = ebeg[k]; e1 = eend[k]; ec = ecnt[k];
    l0 = hrem ? rkoff[k] : 0ull;
    // the key's first batch point inside the range: the combined points before an element of the run are counted from here
    const unsigned long long jf = (b && e1 > e0 && from != 0) ? lower_time(nt, p0, p0 + b, from) : p0;
    rf = (b && e1 > e0) ? roff[jf] : 0ull;
    nrep = (hrem && b) ? roff[p0 + b] - roff[p0] : 0ull;
  }
  const unsigned long long c0 = (w - coff[k]) * kMergeChunk;
  unsigned long long c1 = c0 + kMergeChunk;
  if (c1 > a + b) c1 = a + b;
  [[maybe_unused]] long long ch_min = kNoChange, ch_max = -kNoChange - 1;   // the lane's changed elements: smallest / largest time, how many
  [[maybe_unused]] unsigned ch_n = 0;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    if (u < a) {
      unsigned long long x = sval_old[o0 + u];
      const long long t = st_old[o0 + u];
      unsigned long long shift = 0;
      [[maybe_unused]] unsigned long long rep = 0;
      [[maybe_unused]] bool hit = false;
      if (b) {   // (a key without batch points: no search; without erased points a coalesced copy)
        const unsigned long long j = lower_time(nt, p0, p0 + b, t);
        shift = nhoff[j] - nh0;
        if (j < p0 + b && nt[j] == t && cls[j] == MG_COMBINED) {
          hit = true;
          [[maybe_unused]] const unsigned long long held = x;
          x = merge_value<RULE>(x, nv[j]);
          if constexpr (REPORT)
            if (x != held) { ch_min = t < ch_min ? t : ch_min; ch_max = t > ch_max ? t : ch_max; ++ch_n; }
        }
        if constexpr (RANGED)
          if (u > e0 && u < e1) rep = roff[j] - rf;   // combined points of the key in [e0, u)
      }
      unsigned long long eb = 0;   // erased points of the key before u
      if constexpr (RANGED) {
        if (u >= e0 && u < e1 && !hit) {
          if (hrem) hrem[l0 + nrep + (u - e0) - rep] = x;
          if constexpr (REPORT) { ch_min = t < ch_min ? t : ch_min; ch_max = t > ch_max ? t : ch_max; ++ch_n; }
          continue;
        }
        eb = u <= e0 ? 0ull : (u >= e1 ? ec : (u - e0) - rep);
      }
      sval_new[d0 + u + shift - eb] = x;
      st_new[d0 + u + shift - eb] = t;
    } else {
      const unsigned long long j = p0 + (u - a);
      const uint8_t c = cls[j];
      const unsigned long long y = nv[j];
      if (c == MG_APPENDED || c == MG_INSERTED) {
        const unsigned long long r = rank[j];
        unsigned long long eb = 0;
        if constexpr (RANGED) eb = r <= e0 ? 0ull : (r >= e1 ? ec : (r - e0) - (roff[j] - rf));
        const unsigned long long d = d0 + r - eb + (nhoff[j] - nh0);
        const long long t = nt[j];
        sval_new[d] = y;
        st_new[d] = t;
        if (hadd) hadd[aoff[j]] = y;
        if constexpr (REPORT) { ch_min = t < ch_min ? t : ch_min; ch_max = t > ch_max ? t : ch_max; ++ch_n; }
      } else if (c == MG_COMBINED && hadd) {
        const unsigned long long x = sval_old[o0 + rank[j]];
        // its place among the key's losses, rkoff[k] + (roff[j] - roff[p0]); without a range rkoff[k] == roff[p0]
        hrem[RANGED ? l0 + (roff[j] - roff[p0]) : roff[j]] = x;
        hadd[aoff[j]] = merge_value<RULE>(x, y);
      }
    }
  }
  if constexpr (REPORT) {   // (every lane of the wavefront is here: the loop has no exit but its end)
    for (int d = 32; d >= 1; d >>= 1) {
      const long long omin = __shfl_xor(ch_min, d), omax = __shfl_xor(ch_max, d);
      ch_n += __shfl_xor(ch_n, d);
      ch_min = omin < ch_min ? omin : ch_min;
      ch_max = omax > ch_max ? omax : ch_max;
    }
    if (lane == 0 && ch_n != 0) {
      atomicMin(&since[k], ch_min);
      atomicMax(&cc->max_t, ch_max);
      atomicAdd(&cc->points, (unsigned long long)ch_n);
    }
  }
}

// ---- the change report's per-key passes ----
__global__ __launch_bounds__(kMBlock) void k_merge_report_fill(uint64_t K, long long *__restrict__ since, ChangeCounters *__restrict__ cc) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  if (k < K) since[k] = kNoChange;
  if (k == 0) { cc->points = 0; cc->keys = 0; cc->min_t = kNoChange; cc->max_t = -kNoChange - 1; }
}

// APPEND: every batch point is newer than what its key held and is kept, so key k's changed points are its batch segment.
template <bool APPEND>
__global__ __launch_bounds__(kMBlock) void k_merge_report_keys(uint64_t K, const unsigned long long *__restrict__ poff, const long long *__restrict__ nt,
                                                              long long *__restrict__ since, ChangeCounters *__restrict__ cc) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  long long t0 = kNoChange;
  [[maybe_unused]] long long t1 = -kNoChange - 1;
  if (k < K) {
    if constexpr (APPEND) {
      const unsigned long long p0 = poff[k], p1 = poff[k + 1];
      if (p1 > p0) { t0 = nt[p0]; t1 = nt[p1 - 1]; }
      since[k] = t0;
    } else {
      t0 = since[k];
    }
  }
  count_wave(t0 != kNoChange, lane, &cc->keys);
  for (int d = 32; d >= 1; d >>= 1) {
    const long long omin = __shfl_xor(t0, d);
    t0 = omin < t0 ? omin : t0;
    if constexpr (APPEND) { const long long omax = __shfl_xor(t1, d); t1 = omax > t1 ? omax : t1; }
  }
  if (lane == 0 && t0 != kNoChange) {
    atomicMin(&cc->min_t, t0);
    if constexpr (APPEND) atomicMax(&cc->max_t, t1);
  }
}

// ---- 6. the moments ----
// replay == NULL: no key replays (the in-order path).  The points are read from the candidate series and times.
__global__ __launch_bounds__(kMBlock) void k_merge_moments(uint64_t K, const uint32_t *__restrict__ replay, const unsigned long long *__restrict__ soff_old,
                                                          const unsigned long long *__restrict__ soff_new, const unsigned long long *__restrict__ sval_new,
                                                          const long long *__restrict__ st_new, double alpha, StreamState cur, StreamState next,
                                                          MergeCounters *__restrict__ mc) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  bool touched = false, rp = false;
  if (k < K) {
    StreamAcc a = stream_load(cur, k);
    const unsigned long long olen = soff_old[k + 1] - soff_old[k];
    const unsigned long long n0 = soff_new[k], nlen = soff_new[k + 1] - n0;
    rp = replay != nullptr && replay[k] != 0;
    touched = rp || nlen > olen;
    if (touched) {
      unsigned long long from = olen;
      if (rp) { a = StreamAcc{0u, 0.0, 0.0, 0.0, 0.0, 0ll, false}; from = 0; }
      const double one_minus = 1.0 - alpha;
      for (unsigned long long i = from; i < nlen; ++i) {
        double sg;
        (void)stream_step(a, alpha, one_minus, (double)sval_new[n0 + i], st_new[n0 + i], &sg);
      }
    }
    stream_store(next, k, a);
  }
  count_wave(touched, lane, &mc->keys_touched);
  count_wave(rp, lane, &mc->keys_replayed);
}

// ---- launchers: the structs the driver holds, taken apart here (the kernels keep their __restrict__ pointers) ----
static inline unsigned merge_blocks(uint64_t lanes) { return (unsigned)((lanes + kMBlock - 1) / kMBlock); }

void launch_merge_classify(hipStream_t s, const HistBatch &b, const StateView &old, long long keep_from, const MergePts &mp, MergeCounters *mc) {
  if (b.P_cap == 0) return;
  hipLaunchKernelGGL(k_merge_classify, dim3(merge_blocks(b.P_cap)), dim3(kMBlock), 0, s, b.nk, b.nt, b.P_dev, b.P_cap, old.K, old.soff, old.st, keep_from,
                     mp.cls, mp.rank, mp.f_nh, mp.f_kept, mp.f_hit, mc);
}

void launch_merge_range(hipStream_t s, const HistBatch &b, const StateView &old, const MergePts &mp, const MergeRule &how) {
  if (old.K == 0) return;
  hipLaunchKernelGGL(k_merge_range, dim3(merge_blocks(old.K)), dim3(kMBlock), 0, s, old.K, old.soff, old.st, b.poff, b.nt, mp.roff, how.from, how.to,
                     how.range->ebeg, how.range->eend, how.range->ecnt);
}

void launch_merge_keys(hipStream_t s, const HistBatch &b, const StateView &old, const MergeInto &into, const MergePts &mp, const MergeKeys &mk,
                       const MergeRule &how) {
  const dim3 grid(merge_blocks(old.K + 1)), block(kMBlock);
  if (how.range)
    hipLaunchKernelGGL(k_merge_keys<true>, grid, block, 0, s, old.K, b.poff, mp.nhoff, mp.aoff, mp.roff, mp.cls, old.soff, old.hoff, into.soff, mk.akoff,
                       mk.rkoff, mk.hoff_mid, mk.chunks_s, mk.chunks_h, mk.replay, how.range->ecnt, how.range->eoff, mk.mcnt);
  else
    hipLaunchKernelGGL(k_merge_keys<false>, grid, block, 0, s, old.K, b.poff, mp.nhoff, mp.aoff, mp.roff, mp.cls, old.soff, old.hoff, into.soff, mk.akoff,
                       mk.rkoff, mk.hoff_mid, mk.chunks_s, mk.chunks_h, mk.replay, nullptr, nullptr, nullptr);
}

uint64_t merge_chunks_bound(uint64_t K, uint64_t total_len) { return K + total_len / kMergeChunk + 1; }

template <int RULE, bool RANGED, bool REPORT>
static void launch_series_rule(hipStream_t s, const HistBatch &b, const StateView &old, const MergeInto &into, const MergePts &mp, const MergeKeys &mk,
                             const MergeRule &how) {
  const ReplaceKeys r = RANGED ? *how.range : ReplaceKeys{};   // (the unranged forms read no run)
  const MergeReport rep = REPORT ? *how.report : MergeReport{};
  hipLaunchKernelGGL((k_merge_series<RULE, RANGED, REPORT>), dim3(merge_blocks(merge_chunks_bound(old.K, old.P + b.P_cap) * 64)), dim3(kMBlock), 0, s, mk.coff_s,
                     old.K, old.soff, old.sval, old.st, b.poff, b.nt, b.nv, mp.cls, mp.rank, mp.nhoff, mp.aoff, mp.roff, into.soff, into.sval, into.st,
                     into.hrem ? mp.hadd : nullptr, into.hrem, mk.rkoff, r.ebeg, r.eend, r.ecnt, how.from, rep.since, rep.cc);
}

template <int RULE, bool RANGED>
static void launch_series_as(hipStream_t s, const HistBatch &b, const StateView &old, const MergeInto &into, const MergePts &mp, const MergeKeys &mk,
                             const MergeRule &how) {
  if (how.report) launch_series_rule<RULE, RANGED, true>(s, b, old, into, mp, mk, how);
  else launch_series_rule<RULE, RANGED, false>(s, b, old, into, mp, mk, how);
}

void launch_merge_series(hipStream_t s, const HistBatch &b, const StateView &old, const MergeInto &into, const MergePts &mp, const MergeKeys &mk,
                         const MergeRule &how) {
  if (old.K == 0) return;
  if (how.range) launch_series_as<MERGE_REPLACE, true>(s, b, old, into, mp, mk, how);
  else if (how.replace) launch_series_as<MERGE_REPLACE, false>(s, b, old, into, mp, mk, how);
  else if (how.op_max) launch_series_as<MERGE_MAX, false>(s, b, old, into, mp, mk, how);
  else launch_series_as<MERGE_SUM, false>(s, b, old, into, mp, mk, how);
}

void launch_merge_moments(hipStream_t s, const StateView &old, const MergeInto &into, const uint32_t *replay, double alpha, StreamState next,
                          MergeCounters *mc) {
  if (old.K == 0) return;
  hipLaunchKernelGGL(k_merge_moments, dim3(merge_blocks(old.K)), dim3(kMBlock), 0, s, old.K, replay, old.soff, into.soff, into.sval, into.st, alpha, old.mom,
                     next, mc);
}

void launch_merge_report_fill(hipStream_t s, uint64_t K, const MergeReport &r) {
  hipLaunchKernelGGL(k_merge_report_fill, dim3(merge_blocks(K ? K : 1)), dim3(kMBlock), 0, s, K, r.since, r.cc);
}

void launch_merge_report_keys(hipStream_t s, uint64_t K, const unsigned long long *poff, const long long *nt, const MergeReport &r) {
  if (K == 0) return;
  if (poff) hipLaunchKernelGGL(k_merge_report_keys<true>, dim3(merge_blocks(K)), dim3(kMBlock), 0, s, K, poff, nt, r.since, r.cc);
  else hipLaunchKernelGGL(k_merge_report_keys<false>, dim3(merge_blocks(K)), dim3(kMBlock), 0, s, K, poff, nt, r.since, r.cc);
}

const void *code_anchor_merge() { return reinterpret_cast<const void *>(&k_merge_classify); }

}  // namespace tad
