// tad_keydict.hip — a key dictionary that OUTLIVES the call: key tuples -> dense ids that stay the same from batch to batch.
//
// tad_factorize (tad_factorize.hip) numbers the keys of ONE call: its table is scratch, and a fingerprint match is confirmed against the
// representative row in that call's input columns.  The streaming states (tad_run_stream, tad_state_merge, tad_run_state ...) want key k to be
// the same flow key in every batch for as long as the state lives, so a streaming host kept its own tuple -> id map (a Go map, pandas:
// 1e6-1.5e7 rows/s) in front of an engine that aggregates 7e10 rows/s.  Here the map lives in HBM:
//   table   the slot table of tad_slots.h (which has the protocol: a look with a plain cached load, a claim with ONE compare-and-swap —
//           slot_claim's atomicCAS) — word = fingerprint (high 32 bits of the tuple's hash) << 32 | key id, all ones = empty: exactly
//           tad_factorize's slot, with the id where that one keeps a row, and a word that never changes once claimed;
//   keys    the tuples themselves, because the rows of earlier batches are gone: one RECORD per key id, kd_stride(n_cols) 8-byte words —
//           word 0 the side (0 = a, 1 = b), words 1 .. n_cols the columns, padded to an even count so that a record starts on a 16-byte
//           boundary and is read with 16-byte loads.  A record is at most 80 bytes: a compare touches one 128-byte line, two when the
//           record straddles one (never for 1, 3 or 7 key columns, whose records are 16, 32 and 64 bytes).
// One batch (tad_keydict_encode):
//   1. k_kd_probe: every kept virtual row looks its tuple up.  Hit -> the id goes to the output; miss -> a flag byte, counted per wavefront.
//      The dictionary is only read.  A batch of known tuples ends here: one pass, one synchronisation.
//   2. the misses are factorised among themselves by launch_factorize with the miss flags as its keep masks: batch-local ids in order of
//      first appearance over [side a ++ side b] and the first row of each — deterministic, whatever order the wavefronts run in.
//   3. k_kd_append: one lane per NEW key copies the tuple from its first row into record num_keys_before + j and claims a slot.  New keys
//      are distinct from each other and from every key held, so nothing is compared here.
//   4. k_kd_fix: id = num_keys_before + local id on the miss rows.
// The table never passes load 1/2 (the host grows it BEFORE step 3: k_kd_rehash fills a table of twice the size from the records, and
// the new one is swapped in when that succeeded), so every probe sequence ends at an empty slot and step 3 cannot fail.
// The other direction (tad_keydict_gather: arbitrary ids -> tuples) reads the records only: k_kd_gather.
// Retiring strings (tad_keydict_mark_codes, tad_keydict_recode): k_kd_mark flags the codes a column's keys still hold, k_kd_recode writes
// the records with their columns passed through code remaps; the fresh table is filled from them by k_kd_rehash.
#include "tad_internal.h"
#include "tad_slots.h"

namespace tad {

static constexpr int kKdBlock = 256;
static constexpr int kKdMaxPairs = (kFzMaxCols + 2) / 2;     // 16-byte words of the longest record

// every 16-byte word of the record is loaded before any is compared (one memory round trip, not one per column)
__device__ __forceinline__ void kd_load_record(const unsigned long long *keys, uint64_t id, int pairs, ulonglong2 (&w)[kKdMaxPairs]) {
  const ulonglong2 *r = reinterpret_cast<const ulonglong2 *>(keys + id * (uint64_t)(2 * pairs));
#pragma unroll
  for (int p = 0; p < kKdMaxPairs; ++p) w[p] = p < pairs ? r[p] : ulonglong2{0ull, 0ull};
}
__device__ __forceinline__ uint64_t kd_word(const ulonglong2 (&w)[kKdMaxPairs], int i) { return (i & 1) ? w[i >> 1].y : w[i >> 1].x; }
__device__ __forceinline__ bool kd_same(const unsigned long long *keys, uint64_t id, int pairs, uint64_t side, const long long (&t)[kFzMaxCols], int n_cols) {
  ulonglong2 w[kKdMaxPairs];
  kd_load_record(keys, id, pairs, w);
  bool same = w[0].x == side;
#pragma unroll
  for (int c = 0; c < kFzMaxCols; ++c)
    if (c < n_cols) same = same & (kd_word(w, c + 1) == (uint64_t)t[c]);
  return same;
}

// Step 1.  kInsert: a miss raises miss[v] (0 is written otherwise: the flags are the keep masks of step 2) and is counted; the output of a miss
// row is left to step 4.  !kInsert (tad_keydict_lookup): a miss is TAD_KEY_SKIP.  A word whose id is >= K is never a match (no such word
// exists in a dictionary that every call left normally).
template <bool kInsert>
__global__ __launch_bounds__(kKdBlock) void k_kd_probe(TupleBatch A, const unsigned long long *__restrict__ table, uint64_t mask, const unsigned long long *__restrict__ keys,
                                                       int pairs, uint64_t K, uint64_t *__restrict__ key_a, uint64_t *__restrict__ key_b, uint8_t *__restrict__ miss,
                                                       unsigned long long *__restrict__ n_miss) {
  const uint64_t V = A.n * A.sides;
  uint32_t missed = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; v < V; v += (uint64_t)gridDim.x * kKdBlock) {
    uint64_t id = TAD_KEY_SKIP;
    bool m = false;
    if (tb_kept(A, v)) {
      const uint64_t side = v >= A.n ? 1ull : 0ull;
      long long t[kFzMaxCols];
#pragma unroll
      for (int c = 0; c < kFzMaxCols; ++c) t[c] = c < A.n_cols ? tb_value(A, v, c) : 0ll;
      m = !slot_find(table, mask, tb_hash(side, t, A.n_cols), K, id, [&](uint64_t cand) { return kd_same(keys, cand, pairs, side, t, A.n_cols); });
    }
    if (kInsert) {
      miss[v] = m ? 1 : 0;
      missed += m ? 1u : 0u;
      if (!m) *(v >= A.n ? key_b + (v - A.n) : key_a + v) = id;
    } else {
      *(v >= A.n ? key_b + (v - A.n) : key_a + v) = id;
    }
  }
  if (kInsert) wave_count_add(n_miss, missed);
}

// Step 3: one lane per new key.  first_row[j] = the virtual row where new key j first appears (step 2).  flags |= KD_FLAG_CLUSTER when a
// claim needed a long probe sequence: the host then grows the table after the call (a hint for speed; the claim itself always succeeds).
__global__ __launch_bounds__(kKdBlock) void k_kd_append(TupleBatch A, const uint64_t *__restrict__ first_row, uint64_t m, uint64_t K0, unsigned long long *__restrict__ table,
                                                        uint64_t mask, unsigned long long *__restrict__ keys, int pairs, uint32_t *__restrict__ flags) {
  const uint64_t V = A.n * A.sides;
  for (uint64_t j = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kKdBlock) {
    const uint64_t v = first_row[j];
    if (v >= V) { atomicOr(flags, KD_FLAG_BAD_ROW); continue; }      // (cannot happen: step 2 wrote it)
    const uint64_t side = v >= A.n ? 1ull : 0ull;
    long long t[kFzMaxCols];
#pragma unroll
    for (int c = 0; c < kFzMaxCols; ++c) t[c] = c < A.n_cols ? tb_value(A, v, c) : 0ll;
    unsigned long long *rec = keys + (K0 + j) * (uint64_t)(2 * pairs);
    rec[0] = side;
#pragma unroll
    for (int c = 0; c < kFzMaxCols; ++c)
      if (c < A.n_cols) rec[c + 1] = (unsigned long long)t[c];
    if (((A.n_cols + 1) & 1) != 0) rec[A.n_cols + 1] = 0ull;          // the pad word
    const uint64_t h = tb_hash(side, t, A.n_cols);
    if (slot_claim(table, mask, h, slot_word(h, K0 + j)) > kKdMaxProbe) atomicOr(flags, KD_FLAG_CLUSTER);      // (K0 + j < 2^32 - 1: never the empty word)
  }
}

// Step 4
__global__ __launch_bounds__(kKdBlock) void k_kd_fix(const uint8_t *__restrict__ miss, const uint64_t *__restrict__ loc_a, const uint64_t *__restrict__ loc_b, uint64_t n,
                                                     uint32_t sides, uint64_t K0, uint64_t *__restrict__ key_a, uint64_t *__restrict__ key_b) {
  const uint64_t V = n * sides;
  for (uint64_t v = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; v < V; v += (uint64_t)gridDim.x * kKdBlock) {
    if (miss[v] == 0) continue;
    if (v >= n) key_b[v - n] = K0 + loc_b[v - n];
    else key_a[v] = K0 + loc_a[v];
  }
}

// Records 0 .. K into an EMPTY table (growth; tad_keydict_import).  kCheck (import): two records with the same tuple raise KD_FLAG_DUPLICATE —
// the second one to arrive finds the first one's slot on its probe sequence before any empty slot, since slots are never given up.
template <bool kCheck>
__global__ __launch_bounds__(kKdBlock) void k_kd_rehash(const unsigned long long *__restrict__ keys, int pairs, int n_cols, uint64_t K, unsigned long long *__restrict__ table,
                                                        uint64_t mask, uint32_t *__restrict__ flags) {
  for (uint64_t j = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; j < K; j += (uint64_t)gridDim.x * kKdBlock) {
    ulonglong2 rw[kKdMaxPairs];
    kd_load_record(keys, j, pairs, rw);
    const uint64_t side = rw[0].x;
    long long t[kFzMaxCols];
#pragma unroll
    for (int c = 0; c < kFzMaxCols; ++c) t[c] = c < n_cols ? (long long)kd_word(rw, c + 1) : 0ll;
    const uint64_t h = tb_hash(side, t, n_cols);
    slot_claim(table, mask, h, slot_word(h, j), [&](unsigned long long w) {
      if (kCheck && (w >> 32) == (h >> 32) && (w & 0xffffffffull) != j && (w & 0xffffffffull) < K && kd_same(keys, w & 0xffffffffull, pairs, side, t, n_cols)) {
        atomicOr(flags, KD_FLAG_DUPLICATE);
        return true;
      }
      return false;
    });
  }
}

// tad_keydict_select: one lane per key.  keep[k] = 1 iff the key's side is the wanted one (q.side < 0: either) and, for every term t, the
// byte of mask[t] at the key's value in column col[t] is not 0 — tad_mask_rows' rule on the records instead of on rows.  The record is
// loaded whole (kd_load_record) before any mask byte is read; the term's column is picked by compares, so the record stays in registers;
// the loop over the terms stays rolled (unrolled, eight pointers, lengths and columns at once spill scalar registers).
// A value outside [0, mask_len[t]) raises KD_FLAG_BAD_CODE and reads nothing.  The selected keys are counted with one atomic per workgroup.
__global__ __launch_bounds__(kKdBlock) void k_kd_select(const unsigned long long *__restrict__ keys, int pairs, uint64_t K, KdSelect q, uint8_t *__restrict__ keep,
                                                        unsigned long long *__restrict__ n_sel, uint32_t *__restrict__ flags) {
  __shared__ uint32_t s_cnt[kKdBlock / 64];
  uint32_t mine = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; k < K; k += (uint64_t)gridDim.x * kKdBlock) {
    ulonglong2 w[kKdMaxPairs];
    kd_load_record(keys, k, pairs, w);
    bool ok = q.side < 0 || w[0].x == (uint64_t)q.side;
    bool bad = false;
#pragma unroll 1
    for (int t = 0; t < q.n_terms; ++t) {      // (uniform: the terms are kernel arguments)
      const int col = q.col[t];
      uint64_t v = 0;
#pragma unroll
      for (int c = 0; c < kFzMaxCols; ++c)
        if (col == c) v = kd_word(w, c + 1);
      const bool in = v < q.mask_len[t];       // (a negative value is a huge unsigned one)
      bad |= !in;
      const uint8_t b = in ? q.mask[t][v] : (uint8_t)0;
      ok = ok & (b != 0);
    }
    if (bad) atomicOr(flags, KD_FLAG_BAD_CODE);
    keep[k] = ok ? 1 : 0;
    mine += ok ? 1u : 0u;
  }
  block_count_add(s_cnt, n_sel, mine);
}

// tad_keydict_gather: one lane per asked id.  The record is loaded whole (kd_load_record: 16-byte loads, 64 lanes on up to 64 lines — a
// gather, whatever the kernel does) and stored column by column: consecutive lanes write consecutive 8-byte words of each column, one byte
// each of the sides.  An id >= K (TAD_KEY_SKIP is one) raises KD_FLAG_BAD_ID, reads no record and writes nothing.
__global__ __launch_bounds__(kKdBlock) void k_kd_gather(const unsigned long long *__restrict__ keys, int pairs, int n_cols, uint64_t K, const uint64_t *__restrict__ key_id,
                                                        uint64_t n, KdGatherOut o, uint32_t *__restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kKdBlock) {
    const uint64_t id = key_id[i];
    if (id >= K) { atomicOr(flags, KD_FLAG_BAD_ID); continue; }
    ulonglong2 w[kKdMaxPairs];
    kd_load_record(keys, id, pairs, w);
#pragma unroll
    for (int c = 0; c < kFzMaxCols; ++c)
      if (c < n_cols && o.col[c] != nullptr) o.col[c][i] = (long long)kd_word(w, c + 1);
    if (o.side != nullptr) o.side[i] = (uint8_t)w[0].x;
  }
}

// tad_keydict_mark_codes: one lane per key.  used[v] = 1 for the key's value v in column `col` — a plain byte store; lanes that hit the
// same code store the same value.  The bytes of the codes no key holds are the caller's (zeroed, or kept when it accumulates).  A value
// outside [0, used_len) raises KD_FLAG_BAD_CODE and stores nothing.
__global__ __launch_bounds__(kKdBlock) void k_kd_mark(const unsigned long long *__restrict__ keys, int pairs, uint64_t K, int col, uint8_t *__restrict__ used,
                                                      uint64_t used_len, uint32_t *__restrict__ flags) {
  for (uint64_t k = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; k < K; k += (uint64_t)gridDim.x * kKdBlock) {
    ulonglong2 w[kKdMaxPairs];
    kd_load_record(keys, k, pairs, w);
    uint64_t v = 0;
#pragma unroll
    for (int c = 0; c < kFzMaxCols; ++c)
      if (col == c) v = kd_word(w, c + 1);
    if (v < used_len) used[v] = 1;             // (a negative value is a huge unsigned one)
    else atomicOr(flags, KD_FLAG_BAD_CODE);
  }
}

// ... and the ones of used: the aligned body eight bytes a lane (the non-zero bytes of a word counted without a loop), the bytes in front
// of and behind it singly; counted per wavefront, summed in LDS, one atomic per workgroup, as k_kd_select counts — from at most
// kKdCountBlocks workgroups, because the atomics of a kernel all meet at one address
static constexpr unsigned kKdCountBlocks = 1024;
__global__ __launch_bounds__(kKdBlock) void k_kd_count_used(const uint8_t *__restrict__ used, uint64_t used_len, unsigned long long *__restrict__ n_used) {
  __shared__ uint32_t s_cnt[kKdBlock / 64];
  const uint64_t lead = (8u - (uint32_t)(reinterpret_cast<uintptr_t>(used) & 7u)) & 7u, head = lead < used_len ? lead : used_len;
  const uint64_t words = (used_len - head) >> 3, tail = head + words * 8;
  const unsigned long long *w = reinterpret_cast<const unsigned long long *>(used + head);
  const uint64_t gid = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kKdBlock;
  uint32_t mine = 0;
  for (uint64_t i = gid; i < words; i += stride) {
    const unsigned long long x = w[i], low7 = 0x7f7f7f7f7f7f7f7full;
    mine += (uint32_t)__popcll((((x & low7) + low7) | x) & ~low7);      // bit 7 of a byte: the byte is not 0
  }
  if (gid < head) mine += used[gid] != 0 ? 1u : 0u;
  if (gid < used_len - tail) mine += used[tail + gid] != 0 ? 1u : 0u;
  block_count_add(s_cnt, n_used, mine);
}

// tad_keydict_recode: one lane per key.  For every term t the key's value v in column col[t] becomes remap[t][v]; the record is loaded
// whole, the term's column is picked by compares (the record stays in registers) and the loop over the terms stays rolled, as in
// k_kd_select.  A value outside [0, len[t]) or one mapped to TAD_CODE_NONE (the key still uses a retired string) raises KD_FLAG_BAD_CODE;
// a value that changes raises KD_FLAG_CHANGED (one atomic per wavefront).  keys_new == NULL: the check alone; else record k of keys_new =
// the recoded record.
__global__ __launch_bounds__(kKdBlock) void k_kd_recode(const unsigned long long *__restrict__ keys, int pairs, uint64_t K, KdRecode q,
                                                        unsigned long long *__restrict__ keys_new, uint32_t *__restrict__ flags) {
  bool any_bad = false, any_changed = false;
  for (uint64_t k = (uint64_t)blockIdx.x * kKdBlock + threadIdx.x; k < K; k += (uint64_t)gridDim.x * kKdBlock) {
    ulonglong2 w[kKdMaxPairs];
    kd_load_record(keys, k, pairs, w);
    bool bad = false;
#pragma unroll 1
    for (int t = 0; t < q.n_terms; ++t) {      // (uniform: the terms are kernel arguments)
      const int col = q.col[t];
      uint64_t v = 0;
#pragma unroll
      for (int c = 0; c < kFzMaxCols; ++c)
        if (col == c) v = kd_word(w, c + 1);
      const bool in = v < q.len[t];
      const long long nv = in ? q.remap[t][v] : (long long)TAD_CODE_NONE;
      bad |= nv < 0;
      any_changed |= (uint64_t)nv != v;
#pragma unroll
      for (int c = 0; c < kFzMaxCols; ++c)
        if (col == c) (((c + 1) & 1) ? w[(c + 1) >> 1].y : w[(c + 1) >> 1].x) = (unsigned long long)nv;
    }
    any_bad |= bad;
    if (keys_new != nullptr && !bad) {
      ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(keys_new + k * (uint64_t)(2 * pairs));
#pragma unroll
      for (int p = 0; p < kKdMaxPairs; ++p)
        if (p < pairs) dst[p] = w[p];
    }
  }
  const unsigned long long wb = __ballot(any_bad), wc = __ballot(any_changed);      // one atomic per wavefront
  if ((threadIdx.x & 63) == 0 && (wb | wc) != 0ull) atomicOr(flags, (wb ? KD_FLAG_BAD_CODE : 0u) | (wc ? KD_FLAG_CHANGED : 0u));
}

int kd_stride(int n_cols) { return (n_cols + 2) & ~1; }     // side + columns, padded to an even number of 8-byte words

static dim3 kd_grid(uint64_t items) { const uint64_t b = (items + kKdBlock - 1) / kKdBlock; return dim3((unsigned)(b < 16384 ? (b ? b : 1) : 16384)); }

void launch_kd_probe(hipStream_t s, const TupleBatch &A, const unsigned long long *table, uint64_t slots, const unsigned long long *keys, uint64_t K, uint64_t *key_a,
                     uint64_t *key_b, uint8_t *miss, unsigned long long *n_miss) {
  const uint64_t V = A.n * A.sides;
  const int pairs = kd_stride(A.n_cols) / 2;
  if (miss != nullptr) hipLaunchKernelGGL(k_kd_probe<true>, kd_grid(V), dim3(kKdBlock), 0, s, A, table, slots - 1, keys, pairs, K, key_a, key_b, miss, n_miss);
  else hipLaunchKernelGGL(k_kd_probe<false>, kd_grid(V), dim3(kKdBlock), 0, s, A, table, slots - 1, keys, pairs, K, key_a, key_b, miss, n_miss);
}

void launch_kd_append(hipStream_t s, const TupleBatch &A, const uint64_t *first_row, uint64_t m, uint64_t K0, unsigned long long *table, uint64_t slots,
                      unsigned long long *keys, uint32_t *flags) {
  hipLaunchKernelGGL(k_kd_append, kd_grid(m), dim3(kKdBlock), 0, s, A, first_row, m, K0, table, slots - 1, keys, kd_stride(A.n_cols) / 2, flags);
}

void launch_kd_fix(hipStream_t s, const uint8_t *miss, const uint64_t *loc_a, const uint64_t *loc_b, uint64_t n, uint32_t sides, uint64_t K0, uint64_t *key_a,
                   uint64_t *key_b) {
  hipLaunchKernelGGL(k_kd_fix, kd_grid(n * sides), dim3(kKdBlock), 0, s, miss, loc_a, loc_b, n, sides, K0, key_a, key_b);
}

void launch_kd_rehash(hipStream_t s, const unsigned long long *keys, int n_cols, uint64_t K, unsigned long long *table, uint64_t slots, uint32_t *flags,
                      bool check_duplicates) {
  const int pairs = kd_stride(n_cols) / 2;
  if (check_duplicates) hipLaunchKernelGGL(k_kd_rehash<true>, kd_grid(K), dim3(kKdBlock), 0, s, keys, pairs, n_cols, K, table, slots - 1, flags);
  else hipLaunchKernelGGL(k_kd_rehash<false>, kd_grid(K), dim3(kKdBlock), 0, s, keys, pairs, n_cols, K, table, slots - 1, flags);
}

void launch_kd_select(hipStream_t s, const unsigned long long *keys, int n_cols, uint64_t K, const KdSelect &q, uint8_t *keep, unsigned long long *n_sel,
                      uint32_t *flags) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_kd_select, kd_grid(K), dim3(kKdBlock), 0, s, keys, kd_stride(n_cols) / 2, K, q, keep, n_sel, flags);
}

void launch_kd_gather(hipStream_t s, const unsigned long long *keys, int n_cols, uint64_t K, const uint64_t *key_id, uint64_t n, const KdGatherOut &o, uint32_t *flags) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_kd_gather, kd_grid(n), dim3(kKdBlock), 0, s, keys, kd_stride(n_cols) / 2, n_cols, K, key_id, n, o, flags);
}

void launch_kd_mark(hipStream_t s, const unsigned long long *keys, int n_cols, uint64_t K, int col, uint8_t *used, uint64_t used_len, uint32_t *flags) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_kd_mark, kd_grid(K), dim3(kKdBlock), 0, s, keys, kd_stride(n_cols) / 2, K, col, used, used_len, flags);
}

void launch_kd_count_used(hipStream_t s, const uint8_t *used, uint64_t used_len, unsigned long long *n_used) {
  if (used_len == 0) return;
  const uint64_t b = (used_len / 8 + kKdBlock - 1) / kKdBlock;      // a lane per 8-byte word; at least one workgroup for the bytes at the two ends
  hipLaunchKernelGGL(k_kd_count_used, dim3((unsigned)(b < kKdCountBlocks ? (b ? b : 1) : kKdCountBlocks)), dim3(kKdBlock), 0, s, used, used_len, n_used);
}

void launch_kd_recode(hipStream_t s, const unsigned long long *keys, int n_cols, uint64_t K, const KdRecode &q, unsigned long long *keys_new, uint32_t *flags) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_kd_recode, kd_grid(K), dim3(kKdBlock), 0, s, keys, kd_stride(n_cols) / 2, K, q, keys_new, flags);
}

// one kernel of this translation unit: tad_engine_create resolves it so that the unit's code object is loaded before the first batch
const void *code_anchor_keydict() { return reinterpret_cast<const void *>(&k_kd_fix); }

}  // namespace tad
