// tad_compact.hip — retiring dead keys: tad_state_compact and tad_keydict_compact (include/tad.h, TAD_FEATURE_KEY_RETIRE).
//
// A streaming state and its key dictionary number keys in order of first appearance and never took an id back: with per-connection keys
// the moments, offsets, key records and table slots grew with the keys EVER seen, and every stream batch walks all of them.  A compaction
// drops the keys that are unseen (n == 0: never fed, or emptied by a trim) or idle (last_t < retire_before_t) and renumbers the survivors
// densely, order kept: new id = the number of survivors below.  Nothing is recomputed — a survivor's moments, history, series and times
// are moved as they are, so the compacted state is bit for bit a fresh state that imported the survivors' exports.
//   1. k_compact_mark, one lane per key: live flag, the series / history lengths it keeps (0 for a retired key), their chunk counts
//      (ceil(len / kHistChunk); 0 for an empty segment, so chunk_key and not chunk_key_min1 finds the key), and the counters — unseen
//      keys, idle keys and the idle keys' points — one atomic per counter and wavefront.
//   2. launch_scan of the flags (new ids), of the lengths (the candidate offsets, indexed by OLD key) and of the chunk counts; the host
//      reads the totals once and sizes the candidates.
//   3. k_compact_keys, one lane per old key: a survivor's moments and offsets go to slot j of the candidates; every lane writes remap[k].
//   4. k_compact_copy, one wavefront per kHistChunk elements of a survivor's segment, lanes on consecutive elements: values (and times)
//      to the candidate offsets; once more for the history.  Skipped when only unseen keys went: their segments are empty, so every arena
//      already is the survivors' segments in order.
// The dictionary: k_kd_live flags the records that stay, launch_scan counts the survivors below each, and k_kd_compact checks remap
// against that count — the kept entries must be exactly 0, 1, ..., m - 1 in order, anything else raises the error word — and moves the
// surviving records to their new index with 16-byte loads and stores.  The table is filled from the new records by launch_kd_rehash.
#include "tad_internal.h"

namespace tad {

static constexpr int kCBlock = 256;
static inline unsigned compact_blocks(uint64_t lanes) { return (unsigned)((lanes + kCBlock - 1) / kCBlock); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;   // lane 0 holds the sum
}

// soff / hoff: the state's current series / history offsets (NULL: the state has none, the lengths are 0)
__global__ __launch_bounds__(kCBlock) void k_compact_mark(uint64_t K, const uint32_t *__restrict__ n, const long long *__restrict__ last_t,
                                                         const unsigned long long *__restrict__ soff, const unsigned long long *__restrict__ hoff,
                                                         long long retire_before, uint32_t *__restrict__ live, uint32_t *__restrict__ slen,
                                                         uint32_t *__restrict__ hlen, uint32_t *__restrict__ schunks, uint32_t *__restrict__ hchunks,
                                                         CompactCounters *__restrict__ cc) {
  const uint64_t k = (uint64_t)blockIdx.x * kCBlock + threadIdx.x;
  const bool in = k < K;   // (no early return: the whole wavefront takes part in the ballots and the reduction)
  const uint32_t nk = in ? n[k] : 0u;
  const bool unseen = in && nk == 0;
  const bool idle = in && nk != 0 && retire_before != 0 && last_t[k] < retire_before;
  const bool alive = in && !unseen && !idle;
  if (in) {
    const unsigned long long sl = alive && soff ? soff[k + 1] - soff[k] : 0ull;
    const unsigned long long hl = alive && hoff ? hoff[k + 1] - hoff[k] : 0ull;
    live[k] = alive ? 1u : 0u;
    slen[k] = (uint32_t)sl;
    hlen[k] = (uint32_t)hl;
    schunks[k] = (uint32_t)((sl + kHistChunk - 1) / kHistChunk);
    hchunks[k] = (uint32_t)((hl + kHistChunk - 1) / kHistChunk);
  }
  const unsigned long long n_unseen = (unsigned long long)__popcll(__ballot(unseen));
  const unsigned long long n_idle = (unsigned long long)__popcll(__ballot(idle));
  const unsigned long long dropped = wave_sum(idle ? (unsigned long long)nk : 0ull);
  if ((threadIdx.x & 63) == 0) {
    if (n_unseen) atomicAdd(&cc->unseen, n_unseen);
    if (n_idle) atomicAdd(&cc->idle, n_idle);
    if (dropped) atomicAdd(&cc->dropped, dropped);
  }
}

// newid / sscan / hscan: the scans of live / slen / hlen (K + 1 entries each).  kMove: survivors write slot j of the candidates `next`,
// soff_out, hoff_out (NULL: no such arena), the last old key writes entry m of the offsets; !kMove (nothing retired): remap alone
template <bool kMove>
__global__ __launch_bounds__(kCBlock) void k_compact_keys(uint64_t K, const uint32_t *__restrict__ live, const unsigned long long *__restrict__ newid,
                                                         const unsigned long long *__restrict__ sscan, const unsigned long long *__restrict__ hscan,
                                                         StreamState cur, StreamState next, unsigned long long *__restrict__ soff_out,
                                                         unsigned long long *__restrict__ hoff_out, unsigned long long *__restrict__ remap) {
  const uint64_t k = (uint64_t)blockIdx.x * kCBlock + threadIdx.x;
  if (k >= K) return;
  const unsigned long long j = newid[k];
  const bool alive = live[k] != 0;
  remap[k] = alive ? j : TAD_KEY_SKIP;
  if (!kMove) return;
  if (alive) {
    stream_store(next, j, stream_load(cur, k));
    if (soff_out) soff_out[j] = sscan[k];
    if (hoff_out) hoff_out[j] = hscan[k];
  }
  if (k == K - 1) {   // the end of the last survivor's segments (with no survivor: entry 0 of the one unseen key, already zero)
    const unsigned long long m = newid[K];
    if (soff_out) soff_out[m] = sscan[K];
    if (hoff_out) hoff_out[m] = hscan[K];
  }
}

// One wavefront per chunk of a survivor's segment: off_old the state's offsets, off_new the scan of the retained lengths (both by old key)
__global__ __launch_bounds__(kCBlock) void k_compact_copy(const unsigned long long *__restrict__ coff, uint64_t K,
                                                         const unsigned long long *__restrict__ off_old, const unsigned long long *__restrict__ val_old,
                                                         const long long *__restrict__ t_old, const unsigned long long *__restrict__ off_new,
                                                         unsigned long long *__restrict__ val_new, long long *__restrict__ t_new) {
  const unsigned long long w = ((uint64_t)blockIdx.x * kCBlock + threadIdx.x) >> 6;
  if (w >= coff[K]) return;
  const unsigned lane = threadIdx.x & 63u;
  const uint64_t k = chunk_key(coff, K, w);   // (a retired or empty key has no chunk and is never found)
  const unsigned long long o0 = off_old[k], len = off_new[k + 1] - off_new[k], d0 = off_new[k];
  const unsigned long long c0 = (w - coff[k]) * kHistChunk;
  unsigned long long c1 = c0 + kHistChunk;
  if (c1 > len) c1 = len;
  for (unsigned long long u = c0 + lane; u < c1; u += 64) {
    val_new[d0 + u] = val_old[o0 + u];
    if (t_old) t_new[d0 + u] = t_old[o0 + u];
  }
}

__global__ __launch_bounds__(kCBlock) void k_kd_live(const unsigned long long *__restrict__ remap, uint64_t K, uint32_t *__restrict__ live) {
  const uint64_t k = (uint64_t)blockIdx.x * kCBlock + threadIdx.x;
  if (k < K) live[k] = remap[k] != TAD_KEY_SKIP ? 1u : 0u;
}

// below = the scan of k_kd_live's flags.  A kept entry must equal the number of kept entries below it; keys_new == NULL: the check alone
__global__ __launch_bounds__(kCBlock) void k_kd_compact(const unsigned long long *__restrict__ remap, const unsigned long long *__restrict__ below, uint64_t K,
                                                       const unsigned long long *__restrict__ keys_old, int pairs, unsigned long long *__restrict__ keys_new,
                                                       uint32_t *__restrict__ err) {
  const uint64_t k = (uint64_t)blockIdx.x * kCBlock + threadIdx.x;
  const unsigned long long r = k < K ? remap[k] : TAD_KEY_SKIP;
  const bool kept = r != TAD_KEY_SKIP;
  const bool bad = kept && r != below[k];
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(err, 1u);   // one atomic per wavefront
  if (!kept || bad || keys_new == nullptr) return;
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(keys_old + k * (uint64_t)(2 * pairs));
  ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(keys_new + r * (uint64_t)(2 * pairs));
  for (int p = 0; p < pairs; ++p) dst[p] = src[p];
}

void launch_compact_mark(hipStream_t s, uint64_t K, StreamState cur, const unsigned long long *soff, const unsigned long long *hoff, long long retire_before,
                         uint32_t *live, uint32_t *slen, uint32_t *hlen, uint32_t *schunks, uint32_t *hchunks, CompactCounters *cc) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_compact_mark, dim3(compact_blocks(K)), dim3(kCBlock), 0, s, K, cur.n, cur.last_t, soff, hoff, retire_before, live, slen, hlen, schunks,
                     hchunks, cc);
}

void launch_compact_keys(hipStream_t s, uint64_t K, const uint32_t *live, const unsigned long long *newid, const unsigned long long *sscan,
                         const unsigned long long *hscan, bool move, StreamState cur, StreamState next, unsigned long long *soff_out,
                         unsigned long long *hoff_out, unsigned long long *remap) {
  if (K == 0) return;
  const dim3 grid(compact_blocks(K)), block(kCBlock);
  if (move) hipLaunchKernelGGL(k_compact_keys<true>, grid, block, 0, s, K, live, newid, sscan, hscan, cur, next, soff_out, hoff_out, remap);
  else hipLaunchKernelGGL(k_compact_keys<false>, grid, block, 0, s, K, live, newid, sscan, hscan, cur, next, soff_out, hoff_out, remap);
}

void launch_compact_copy(hipStream_t s, uint64_t chunks, const unsigned long long *coff, uint64_t K, const unsigned long long *off_old,
                         const unsigned long long *val_old, const long long *t_old, const unsigned long long *off_new, unsigned long long *val_new,
                         long long *t_new) {
  if (K == 0 || chunks == 0) return;
  hipLaunchKernelGGL(k_compact_copy, dim3(compact_blocks(chunks * 64)), dim3(kCBlock), 0, s, coff, K, off_old, val_old, t_old, off_new, val_new, t_new);
}

void launch_kd_live(hipStream_t s, const unsigned long long *remap, uint64_t K, uint32_t *live) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_kd_live, dim3(compact_blocks(K)), dim3(kCBlock), 0, s, remap, K, live);
}

void launch_kd_compact(hipStream_t s, const unsigned long long *remap, const unsigned long long *below, uint64_t K, const unsigned long long *keys_old,
                       int n_cols, unsigned long long *keys_new, uint32_t *err) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_kd_compact, dim3(compact_blocks(K)), dim3(kCBlock), 0, s, remap, below, K, keys_old, kd_stride(n_cols) / 2, keys_new, err);
}

const void *code_anchor_compact() { return reinterpret_cast<const void *>(&k_compact_mark); }

}  // namespace tad
