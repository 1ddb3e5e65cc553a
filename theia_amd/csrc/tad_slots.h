// tad_slots.h — the slot table of the four ingest encoders (tad_factorize, tad_encode_strings: the keys of one call; tad_keydict,
// tad_strdict: ids that outlive the call), and what their kernels share beside it: the hash's finaliser, the tuple batch's accessors and
// the two ways a kernel counts.  Device code only, included by tad_keydict.hip and by tad_strbytes.h (and through it by tad_factorize.hip
// and tad_strdict.hip).
//
// The table: open addressing, linear probing, one 8-byte word per slot
//     word = fingerprint (the high 32 bits of the key's hash) << 32 | id          (all ones = empty)
// where id is whatever the encoder numbers its keys by (a representative row, a key id, a code; always < 2^32 - 1, so a word is never the
// empty one).  A slot is claimed with ONE compare-and-swap (atomicCAS): fingerprint and id appear together, no reader ever sees a
// half-written slot and nobody spins.  A claimed slot's fingerprint never changes.
#pragma once
#include "tad_internal.h"

namespace tad {

static constexpr unsigned long long kSlotEmpty = ~0ull;

// A probe LOOKS at a slot with a plain cached load.  On this multi-XCD chip an agent-scope load is a transaction with the memory side for every
// row (the L2s of the eight XCDs are not coherent with each other, so device-scope accesses bypass them): 1e8 of them were the insert pass
// (3 of its 4 ms for one key column, profiles/r4_v29_*).  A stale view is harmless here: a slot's fingerprint never changes once claimed, so a
// non-empty word is trusted for WHICH slot it is (where the low half may still move — tad_factorize's atomic min — it may be stale-high: the
// min is then merely redundant), and a word that looks empty is only ever claimed with a compare-and-swap, which is performed at the memory
// side and returns the truth.  So a stale view can only show "empty" where a slot has just been claimed, and the claim sees through it.
__device__ __forceinline__ unsigned long long slot_peek(const unsigned long long *slot) {
  return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ unsigned long long slot_word(uint64_t h, uint64_t id) { return ((h >> 32) << 32) | id; }

__device__ __forceinline__ uint64_t fz_mix(uint64_t x) {   // splitmix64 finaliser
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Claim the first empty slot on h's probe sequence for `word` (a key that no slot holds yet: nothing is compared).  -> the slots passed over.
// occupied(w): called with every word met on the way; true ends the walk without a claim (k_kd_rehash's duplicate check).
// The table must have an empty slot (the dictionaries keep the load <= 1/2).
template <class Occupied>
__device__ __forceinline__ uint32_t slot_claim(unsigned long long *table, uint64_t mask, uint64_t h, unsigned long long word, Occupied occupied) {
  uint32_t probes = 0;
  for (uint64_t s = h & mask;; s = (s + 1) & mask, ++probes) {
    unsigned long long w = slot_peek(table + s);
    if (w == kSlotEmpty) {
      w = atomicCAS(table + s, kSlotEmpty, word);
      if (w == kSlotEmpty) break;                                      // claimed
    }
    if (occupied(w)) break;
  }
  return probes;
}
__device__ __forceinline__ uint32_t slot_claim(unsigned long long *table, uint64_t mask, uint64_t h, unsigned long long word) {
  return slot_claim(table, mask, h, word, [](unsigned long long) { return false; });
}

// Is the key with hash h among the K ids held?  -> true and id = its id; false (a miss) and id as it was.  same(cand): the key IS cand's (a
// fingerprint match alone is not equality).  A word whose id is >= K is never a match.  (load <= 1/2: every probe sequence reaches an empty slot)
template <class Same>
__device__ __forceinline__ bool slot_find(const unsigned long long *table, uint64_t mask, uint64_t h, uint64_t K, uint64_t &id, Same same) {
  for (uint64_t s = h & mask;; s = (s + 1) & mask) {
    const unsigned long long w = slot_peek(table + s);
    if (w == kSlotEmpty) return false;
    const uint64_t cand = w & 0xffffffffull;
    if ((w >> 32) == (h >> 32) && cand < K && same(cand)) { id = cand; return true; }
  }
}

// *counter += the sum of n over the wavefront: one atomic per wavefront (every lane of the workgroup calls this, once, at the kernel's end)
__device__ __forceinline__ void wave_count_add(unsigned long long *counter, uint32_t n) {
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (unsigned long long)n);
}
// ... over the workgroup: summed per wavefront, then per workgroup in LDS (s_cnt: one entry per wavefront), one atomic per workgroup
template <int kWaves>
__device__ __forceinline__ void block_count_add(uint32_t (&s_cnt)[kWaves], unsigned long long *counter, uint32_t n) {
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) total += s_cnt[i];
    if (total) atomicAdd(counter, (unsigned long long)total);
  }
}

// ---- a TupleBatch's virtual rows [side a: 0 .. n) ++ [side b: n .. 2n) ----
__device__ __forceinline__ bool tb_kept(const TupleBatch &A, uint64_t v) {
  const bool sb = v >= A.n;
  const uint8_t *keep = sb ? A.keep_b : A.keep_a;
  return keep == nullptr || keep[sb ? v - A.n : v] != 0;
}
__device__ __forceinline__ long long tb_value(const TupleBatch &A, uint64_t v, int c) {
  const bool sb = v >= A.n;
  return (sb ? A.b[c] : A.a[c])[sb ? v - A.n : v];
}
// THE hash of a key tuple — tad_factorize's table, the key dictionary's table and its exported records all rest on it — column by column:
// from kTupleSideB or 0 (the side is part of the tuple), tb_hash_col for the columns 0 .. n_cols - 1 in order, fz_mix at the end.  Two loops
// are built on it, because one loop form does not serve every kernel: k_fz_insert fetches a column as it hashes it in a ROLLED loop
// (unrolled it loses a wavefront per SIMD), the dictionary's kernels hash the tuple they hold with tb_hash, UNROLLED (rolled, the compiler
// indexes k_kd_rehash's record dynamically and moves it to 20 KB of LDS).
static constexpr uint64_t kTupleSideB = 0x9E3779B97F4A7C15ull;      // the hash starts from this on side b, from 0 on side a
__device__ __forceinline__ uint64_t tb_hash_col(uint64_t h, long long x, int c) { return fz_mix(h ^ (uint64_t)x) + 0x632BE59BD9B4E019ull * (uint64_t)(c + 1); }
__device__ __forceinline__ uint64_t tb_hash(uint64_t side, const long long (&t)[kFzMaxCols], int n_cols) {
  uint64_t h = side ? kTupleSideB : 0ull;
#pragma unroll
  for (int c = 0; c < kFzMaxCols; ++c)
    if (c < n_cols) h = tb_hash_col(h, t[c], c);
  return fz_mix(h);
}

}  // namespace tad
