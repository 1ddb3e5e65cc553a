// tad_merge.hip — a batch placed BY TIME into a streaming state that keeps its series with times (include/tad.h: tad_state_merge).
//
// tad_run_stream appends: a row not newer than its key's last point fails the batch.  A merge takes the same batch — Stage 0's points in
// (key, time) order, nk / nt / nv with poff[K + 1], as a history batch has them (tad_history.hip) — and puts every point where its time
// says, into the candidate copies of the state:
//   1. k_merge_classify, one lane per batch point: too old (before keep_from), appended (newer than everything the key holds), combined
//      (a time the key already holds: found by a lower_bound in the key's old times) or inserted (a new time in between); rank = the old
//      points of the key before it.  Three flag arrays for the scans, the call's counters with one atomic per wavefront.
//   2. scans over the points (launch_scan): nhoff = the points that add an element (inserted / appended), aoff = the kept points (what the
//      history gains), roff = the combined points (what the history loses); k_merge_keys turns them into the per-key candidate series
//      offsets, the packed per-key offsets of the history's gains and losses, and the chunk counts of 3 and 4.
//   3. k_merge_series, a wavefront per kMergeChunk elements of a key's [old segment | batch points] as k_hist_merge: old element u goes to
//      u + #{batch points of the key before its time that add an element}, its value op(old, new) where a batch point hit it; a batch point
//      that adds an element goes to rank + its index among those.  Values and times are written together; a key without batch points is a
//      coalesced copy.  History states: the same lanes pack the values the history loses (old values of combined points) and gains.
//   4. the history: both packed lists sorted per key (launch_hist_sort), launch_hist_subtract into a scratch arena, launch_hist_merge into
//      the candidate (tad_history.hip; the host skips the subtract when nothing combined).
//   5. k_merge_moments, one lane per key: a key with an inserted or combined point is replayed from the zero state over its merged series
//      (stream_step: the fresh state's bits), a key that only gained newer points continues from its stored state, the rest is copied.
// Times inside one key's batch segment ascend strictly (Stage 0 made the points unique), as the key's old times do.
#include <stdint.h>

#include "tad_internal.h"

namespace tad {

static constexpr int kMBlock = 256;
static constexpr uint32_t kMergeChunk = 2048;   // k_merge_series: elements per wavefront (32 per lane), as k_hist_merge

// (the classes MG_*, lower_time and count_wave are in tad_internal.h: tad_replace.hip shares them)

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

// ---- 2. per key: candidate offsets, packed history offsets, chunk counts, who replays ----
// One lane per k <= K.  The kept points of a key are a suffix of its batch segment (the too-old ones come first in time), and a key whose
// first kept point is newer than its last old point has only such points: replay[k] = the first kept point is inserted or combined.
__global__ __launch_bounds__(kMBlock) void k_merge_keys(uint64_t K, const unsigned long long *__restrict__ poff, const unsigned long long *__restrict__ nhoff,
                                                       const unsigned long long *__restrict__ aoff, const unsigned long long *__restrict__ roff,
                                                       const uint8_t *__restrict__ cls, const unsigned long long *__restrict__ soff_old,
                                                       const unsigned long long *__restrict__ hoff_old, unsigned long long *__restrict__ soff_new,
                                                       unsigned long long *__restrict__ akoff, unsigned long long *__restrict__ rkoff,
                                                       unsigned long long *__restrict__ hoff_mid, uint32_t *__restrict__ chunks_s,
                                                       uint32_t *__restrict__ chunks_h, uint32_t *__restrict__ replay) {
  const uint64_t k = (uint64_t)blockIdx.x * kMBlock + threadIdx.x;
  if (k > K) return;
  const unsigned long long p0 = poff[k];
  soff_new[k] = soff_old[k] + nhoff[p0];
  if (hoff_old) {
    akoff[k] = aoff[p0];
    rkoff[k] = roff[p0];
    hoff_mid[k] = hoff_old[k] - roff[p0];
  }
  if (k == K) return;
  const unsigned long long p1 = poff[k + 1];
  const unsigned long long len = (soff_old[k + 1] - soff_old[k]) + (p1 - p0);
  chunks_s[k] = (uint32_t)((len + kMergeChunk - 1) / kMergeChunk);
  if (hoff_old) chunks_h[k] = (uint32_t)((hoff_old[k + 1] - hoff_old[k] + kMergeChunk - 1) / kMergeChunk);
  const unsigned long long kept = aoff[p1] - aoff[p0];
  replay[k] = (kept != 0 && cls[p1 - kept] != MG_APPENDED) ? 1u : 0u;
}

// ---- 3. the series and its times merged by time ----
template <bool OP_MAX>
__global__ __launch_bounds__(kMBlock) void k_merge_series(const unsigned long long *__restrict__ coff, uint64_t K,
                                                         const unsigned long long *__restrict__ soff_old, const unsigned long long *__restrict__ sval_old,
                                                         const long long *__restrict__ st_old, const unsigned long long *__restrict__ poff,
                                                         const long long *__restrict__ nt, const unsigned long long *__restrict__ nv,
                                                         const uint8_t *__restrict__ cls, const uint32_t *__restrict__ rank,
                                                         const unsigned long long *__restrict__ nhoff, const unsigned long long *__restrict__ aoff,
                                                         const unsigned long long *__restrict__ roff, const unsigned long long *__restrict__ soff_new,
                                                         unsigned long long *__restrict__ sval_new, long long *__restrict__ st_new,
                                                         unsigned long long *__restrict__ hadd, unsigned long long *__restrict__ hrem) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kMBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  uint64_t lo = 0, hi = K;   // the key of wavefront w (wavefront-uniform): the last k with coff[k] <= w
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (coff[mid] <= w) lo = mid; else hi = mid; }
  const uint64_t k = lo;
  const unsigned long long o0 = soff_old[k], a = soff_old[k + 1] - o0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  const unsigned long long d0 = soff_new[k];
  const unsigned long long nh0 = b ? nhoff[p0] : 0ull;
  const unsigned long long c0 = (w - coff[k]) * kMergeChunk;
  unsigned long long c1 = c0 + kMergeChunk;
  if (c1 > a + b) c1 = a + b;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    if (u < a) {
      unsigned long long x = sval_old[o0 + u];
      const long long t = st_old[o0 + u];
      unsigned long long shift = 0;
      if (b) {   // (a key without batch points: a coalesced copy)
        const unsigned long long j = lower_time(nt, p0, p0 + b, t);
        shift = nhoff[j] - nh0;
        if (j < p0 + b && nt[j] == t && cls[j] == MG_COMBINED) {
          const unsigned long long y = nv[j];
          x = OP_MAX ? (x > y ? x : y) : x + y;
        }
      }
      sval_new[d0 + u + shift] = x;
      st_new[d0 + u + shift] = t;
    } else {
      const unsigned long long j = p0 + (u - a);
      const uint8_t c = cls[j];
      const unsigned long long y = nv[j];
      if (c == MG_APPENDED || c == MG_INSERTED) {
        const unsigned long long d = d0 + rank[j] + (nhoff[j] - nh0);
        sval_new[d] = y;
        st_new[d] = nt[j];
        if (hadd) hadd[aoff[j]] = y;
      } else if (c == MG_COMBINED && hadd) {
        const unsigned long long x = sval_old[o0 + rank[j]];
        hrem[roff[j]] = x;
        hadd[aoff[j]] = OP_MAX ? (x > y ? x : y) : x + y;
      }
    }
  }
}

// ---- 5. the moments ----
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

// ---- launchers ----
static inline unsigned merge_blocks(uint64_t lanes) { return (unsigned)((lanes + kMBlock - 1) / kMBlock); }

void launch_merge_classify(hipStream_t s, const unsigned long long *nk, const long long *nt, const unsigned long long *P_dev, uint64_t P_cap, uint64_t K,
                           const unsigned long long *soff, const long long *st, long long keep_from, uint8_t *cls, uint32_t *rank, uint32_t *f_nh,
                           uint32_t *f_kept, uint32_t *f_hit, MergeCounters *mc) {
  if (P_cap == 0) return;
  hipLaunchKernelGGL(k_merge_classify, dim3(merge_blocks(P_cap)), dim3(kMBlock), 0, s, nk, nt, P_dev, P_cap, K, soff, st, keep_from, cls, rank, f_nh, f_kept,
                     f_hit, mc);
}

void launch_merge_keys(hipStream_t s, uint64_t K, const unsigned long long *poff, const unsigned long long *nhoff, const unsigned long long *aoff,
                       const unsigned long long *roff, const uint8_t *cls, const unsigned long long *soff_old, const unsigned long long *hoff_old,
                       unsigned long long *soff_new, unsigned long long *akoff, unsigned long long *rkoff, unsigned long long *hoff_mid, uint32_t *chunks_s,
                       uint32_t *chunks_h, uint32_t *replay) {
  hipLaunchKernelGGL(k_merge_keys, dim3(merge_blocks(K + 1)), dim3(kMBlock), 0, s, K, poff, nhoff, aoff, roff, cls, soff_old, hoff_old, soff_new, akoff, rkoff,
                     hoff_mid, chunks_s, chunks_h, replay);
}

uint64_t merge_chunks_bound(uint64_t K, uint64_t total_len) { return K + total_len / kMergeChunk + 1; }

void launch_merge_series(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, bool op_max, const unsigned long long *soff_old,
                         const unsigned long long *sval_old, const long long *st_old, const unsigned long long *poff, const long long *nt,
                         const unsigned long long *nv, const uint8_t *cls, const uint32_t *rank, const unsigned long long *nhoff,
                         const unsigned long long *aoff, const unsigned long long *roff, const unsigned long long *soff_new, unsigned long long *sval_new,
                         long long *st_new, unsigned long long *hadd, unsigned long long *hrem) {
  if (K == 0) return;
  const dim3 grid(merge_blocks(chunks_bound * 64)), block(kMBlock);
  if (op_max)
    hipLaunchKernelGGL(k_merge_series<true>, grid, block, 0, s, coff, K, soff_old, sval_old, st_old, poff, nt, nv, cls, rank, nhoff, aoff, roff, soff_new,
                       sval_new, st_new, hadd, hrem);
  else
    hipLaunchKernelGGL(k_merge_series<false>, grid, block, 0, s, coff, K, soff_old, sval_old, st_old, poff, nt, nv, cls, rank, nhoff, aoff, roff, soff_new,
                       sval_new, st_new, hadd, hrem);
}

void launch_merge_moments(hipStream_t s, uint64_t K, const uint32_t *replay, const unsigned long long *soff_old, const unsigned long long *soff_new,
                          const unsigned long long *sval_new, const long long *st_new, double alpha, StreamState cur, StreamState next, MergeCounters *mc) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_merge_moments, dim3(merge_blocks(K)), dim3(kMBlock), 0, s, K, replay, soff_old, soff_new, sval_new, st_new, alpha, cur, next, mc);
}

const void *code_anchor_merge() { return reinterpret_cast<const void *>(&k_merge_classify); }

}  // namespace tad
