// tad_replace.hip — a batch that REPLACES what a streaming state holds (include/tad.h: tad_state_replace).
//
// tad_state_merge (tad_merge.hip) combines a batch point with the point its key already holds at that time; a re-read of the same rows
// under sum then doubles them.  A replace takes the same batch — Stage 0's points in (key, time) order, nk / nt / nv with poff[K + 1] —
// and makes it the truth: a point at a held time takes the batch's value, and with a range R = [from, to) every old point of EVERY key
// inside R that the batch does not name is erased.  The shape is the merge's, and the classification is the merge's own kernel
// (k_merge_classify: "combined" reads "replaced" here), as are the scans, the history kernels and the moments:
//   1. k_merge_classify, lane per batch point; the scans nhoff (adds an element), aoff (kept), roff (replaced).
//   2. k_replace_range, lane per key: the erased run [e0, e1) of the key's old segment — two lower_bounds in its times — and
//      ecnt = (e1 - e0) - the replaced points of the key inside the run (two lower_bounds in its batch segment, a difference of roff);
//      eoff = the scan of ecnt.
//   3. k_replace_keys, lane per k <= K: soff_new = soff_old + nhoff[p0] - eoff; the packed history gains at aoff[p0], the losses (replaced
//      and erased) at roff[p0] + eoff; chunk counts on a + b; replay = the key has an inserted, replaced or erased point; keys emptied.
//   4. k_replace_series, a wavefront per kMergeChunk elements of a key's [old segment | batch points]: an old element inside the run that
//      no batch point hits is dropped (its value to the history's losses); any other goes to u + added_before(u) - erased_before(u) with
//      the batch's value where it is hit; a batch point that adds an element goes to rank - erased_before(rank) + its index among those.
//      A key without batch points and without erased points is a coalesced copy.
//   5. the history: launch_hist_sort of both packed lists, launch_hist_subtract into the scratch arena, launch_hist_merge (tad_history.hip).
//   6. k_merge_moments with the new replay flags: a replayed key starts from the zero state, so an emptied key holds an unseen key's bits.
// No LDS, no scratch.  Times inside one key's batch segment ascend strictly, as the key's old times do.
#include <stdint.h>

#include "tad_internal.h"

namespace tad {

static constexpr int kRBlock = 256;
static constexpr uint32_t kReplaceChunk = 2048;   // k_replace_series: elements per wavefront, k_merge_series' kMergeChunk

// ---- 2. per key: the erased run and what it loses ----
// from / to == 0: no bound on that side.  A replaced point's time is an old time, so the replaced points with rank in [e0, e1) are the
// replaced batch points with time in [from, to): roff[jt] - roff[jf].
__global__ __launch_bounds__(kRBlock) void k_replace_range(uint64_t K, const unsigned long long *__restrict__ soff, const long long *__restrict__ st,
                                                          const unsigned long long *__restrict__ poff, const long long *__restrict__ nt,
                                                          const unsigned long long *__restrict__ roff, long long from, long long to,
                                                          uint32_t *__restrict__ ebeg, uint32_t *__restrict__ eend, uint32_t *__restrict__ ecnt) {
  const uint64_t k = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
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
// As k_merge_keys; the kept points of a key are a suffix of its batch segment, so replay[k] = the first kept point is inserted or
// replaced, or the key lost a point to the range.
__global__ __launch_bounds__(kRBlock) void k_replace_keys(uint64_t K, const unsigned long long *__restrict__ poff, const unsigned long long *__restrict__ nhoff,
                                                         const unsigned long long *__restrict__ aoff, const unsigned long long *__restrict__ roff,
                                                         const uint8_t *__restrict__ cls, const uint32_t *__restrict__ ecnt,
                                                         const unsigned long long *__restrict__ eoff, const unsigned long long *__restrict__ soff_old,
                                                         const unsigned long long *__restrict__ hoff_old, unsigned long long *__restrict__ soff_new,
                                                         unsigned long long *__restrict__ akoff, unsigned long long *__restrict__ rkoff,
                                                         unsigned long long *__restrict__ hoff_mid, uint32_t *__restrict__ chunks_s,
                                                         uint32_t *__restrict__ chunks_h, uint32_t *__restrict__ replay, MergeCounters *__restrict__ mc) {
  const uint64_t k = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  bool emptied = false;
  if (k <= K) {
    const unsigned long long p0 = poff[k], eo = eoff[k];
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
    chunks_s[k] = (uint32_t)((len + kReplaceChunk - 1) / kReplaceChunk);
    if (hoff_old) chunks_h[k] = (uint32_t)((hoff_old[k + 1] - hoff_old[k] + kHistChunk - 1) / kHistChunk);
    const unsigned long long kept = aoff[p1] - aoff[p0];
    const uint32_t ec = ecnt[k];
    replay[k] = ((kept != 0 && cls[p1 - kept] != MG_APPENDED) || ec != 0) ? 1u : 0u;
    emptied = a != 0 && a + (nhoff[p1] - nhoff[p0]) == (unsigned long long)ec;
  }
  count_wave(emptied, lane, &mc->keys_emptied);
}

// ---- 4. the series and its times: erased, replaced, inserted, appended ----
__global__ __launch_bounds__(kRBlock) void k_replace_series(const unsigned long long *__restrict__ coff, uint64_t K,
                                                           const unsigned long long *__restrict__ soff_old, const unsigned long long *__restrict__ sval_old,
                                                           const long long *__restrict__ st_old, const unsigned long long *__restrict__ poff,
                                                           const long long *__restrict__ nt, const unsigned long long *__restrict__ nv,
                                                           const uint8_t *__restrict__ cls, const uint32_t *__restrict__ rank,
                                                           const unsigned long long *__restrict__ nhoff, const unsigned long long *__restrict__ aoff,
                                                           const unsigned long long *__restrict__ roff, const uint32_t *__restrict__ ebeg,
                                                           const uint32_t *__restrict__ eend, const uint32_t *__restrict__ ecnt, long long from,
                                                           const unsigned long long *__restrict__ rkoff, const unsigned long long *__restrict__ soff_new,
                                                           unsigned long long *__restrict__ sval_new, long long *__restrict__ st_new,
                                                           unsigned long long *__restrict__ hadd, unsigned long long *__restrict__ hrem) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kRBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key(coff, K, w);   // (wavefront-uniform; a key without elements has no chunk)
  const unsigned long long o0 = soff_old[k], a = soff_old[k + 1] - o0;
  const unsigned long long p0 = poff[k], b = poff[k + 1] - p0;
  const unsigned long long d0 = soff_new[k];
  const unsigned long long e0 = ebeg[k], e1 = eend[k], ec = ecnt[k];
  const unsigned long long nh0 = b ? nhoff[p0] : 0ull;
  // the key's first batch point inside the range: the replaced points before an element of the run are counted from here
  const unsigned long long jf = (b && e1 > e0) ? (from != 0 ? lower_time(nt, p0, p0 + b, from) : p0) : p0;
  const unsigned long long rf = (b && e1 > e0) ? roff[jf] : 0ull;
  // the key's losses in the packed list: its replaced points' old values first, then its erased points in time order
  const unsigned long long l0 = hrem ? rkoff[k] : 0ull;
  const unsigned long long nrep = (hrem && b) ? roff[p0 + b] - roff[p0] : 0ull;
  const unsigned long long c0 = (w - coff[k]) * kReplaceChunk;
  unsigned long long c1 = c0 + kReplaceChunk;
  if (c1 > a + b) c1 = a + b;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    if (u < a) {
      unsigned long long x = sval_old[o0 + u];
      const long long t = st_old[o0 + u];
      unsigned long long shift = 0, rep = 0;
      bool hit = false;
      if (b) {   // (a key without batch points: no search)
        const unsigned long long j = lower_time(nt, p0, p0 + b, t);
        shift = nhoff[j] - nh0;
        hit = j < p0 + b && nt[j] == t && cls[j] == MG_COMBINED;
        if (hit) x = nv[j];
        if (u > e0 && u < e1) rep = roff[j] - rf;   // replaced points of the key in [e0, u)
      }
      const bool in_run = u >= e0 && u < e1;
      if (in_run && !hit) {
        if (hrem) hrem[l0 + nrep + (u - e0) - rep] = x;
      } else {
        const unsigned long long eb = u <= e0 ? 0ull : (u >= e1 ? ec : (u - e0) - rep);
        sval_new[d0 + u + shift - eb] = x;
        st_new[d0 + u + shift - eb] = t;
      }
    } else {
      const unsigned long long j = p0 + (u - a);
      const uint8_t c = cls[j];
      const unsigned long long y = nv[j];
      if (c == MG_APPENDED || c == MG_INSERTED) {
        const unsigned long long r = rank[j];
        const unsigned long long eb = r <= e0 ? 0ull : (r >= e1 ? ec : (r - e0) - (roff[j] - rf));
        const unsigned long long d = d0 + r - eb + (nhoff[j] - nh0);
        sval_new[d] = y;
        st_new[d] = nt[j];
        if (hadd) hadd[aoff[j]] = y;
      } else if (c == MG_COMBINED && hadd) {
        hrem[l0 + (roff[j] - roff[p0])] = sval_old[o0 + rank[j]];
        hadd[aoff[j]] = y;
      }
    }
  }
}

// ---- launchers ----
static inline unsigned replace_blocks(uint64_t lanes) { return (unsigned)((lanes + kRBlock - 1) / kRBlock); }

void launch_replace_range(hipStream_t s, uint64_t K, const unsigned long long *soff, const long long *st, const unsigned long long *poff, const long long *nt,
                          const unsigned long long *roff, long long from, long long to, uint32_t *ebeg, uint32_t *eend, uint32_t *ecnt) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_replace_range, dim3(replace_blocks(K)), dim3(kRBlock), 0, s, K, soff, st, poff, nt, roff, from, to, ebeg, eend, ecnt);
}

void launch_replace_keys(hipStream_t s, uint64_t K, const unsigned long long *poff, const unsigned long long *nhoff, const unsigned long long *aoff,
                         const unsigned long long *roff, const uint8_t *cls, const uint32_t *ecnt, const unsigned long long *eoff,
                         const unsigned long long *soff_old, const unsigned long long *hoff_old, unsigned long long *soff_new, unsigned long long *akoff,
                         unsigned long long *rkoff, unsigned long long *hoff_mid, uint32_t *chunks_s, uint32_t *chunks_h, uint32_t *replay, MergeCounters *mc) {
  hipLaunchKernelGGL(k_replace_keys, dim3(replace_blocks(K + 1)), dim3(kRBlock), 0, s, K, poff, nhoff, aoff, roff, cls, ecnt, eoff, soff_old, hoff_old, soff_new,
                     akoff, rkoff, hoff_mid, chunks_s, chunks_h, replay, mc);
}

void launch_replace_series(hipStream_t s, uint64_t chunks_bound, const unsigned long long *coff, uint64_t K, const unsigned long long *soff_old,
                           const unsigned long long *sval_old, const long long *st_old, const unsigned long long *poff, const long long *nt,
                           const unsigned long long *nv, const uint8_t *cls, const uint32_t *rank, const unsigned long long *nhoff,
                           const unsigned long long *aoff, const unsigned long long *roff, const uint32_t *ebeg, const uint32_t *eend, const uint32_t *ecnt,
                           long long from, const unsigned long long *rkoff, const unsigned long long *soff_new, unsigned long long *sval_new,
                           long long *st_new, unsigned long long *hadd, unsigned long long *hrem) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_replace_series, dim3(replace_blocks(chunks_bound * 64)), dim3(kRBlock), 0, s, coff, K, soff_old, sval_old, st_old, poff, nt, nv, cls,
                     rank, nhoff, aoff, roff, ebeg, eend, ecnt, from, rkoff, soff_new, sval_new, st_new, hadd, hrem);
}

const void *code_anchor_replace() { return reinterpret_cast<const void *>(&k_replace_range); }

}  // namespace tad
