// tad_strdict.hip — a string dictionary that OUTLIVES the call: the strings of an Arrow column -> codes that stay the same from batch to batch.
//
// tad_encode_strings (tad_factorize.hip) numbers the strings of ONE call: its table is scratch, and a fingerprint match is confirmed against
// the representative row in that call's own bytes.  A streaming host wants string s to be the same code in every batch for as long as the
// key dictionary behind it lives (tad.h, tad_keydict: "one vocabulary per column, kept for the life of the dictionary"), so it kept its own
// string -> code map (numpy's unique + a Python dict per batch and column) in front of an encode that runs at 2.3e10 rows/s.  Here the map
// lives in HBM — to tad_encode_strings what tad_keydict.hip is to tad_factorize:
//   table    the slot table of tad_slots.h (which has the protocol: a look with a plain cached load, a claim with ONE compare-and-swap —
//            slot_claim's atomicCAS) — word = fingerprint (high 32 bits of the string's hash) << 32 | code, all ones = empty, and a word
//            that never changes once claimed;
//   records  one 16-byte record per code, read with one 16-byte load: the string's offset in the arena (8 bytes), its length (4) and the LOW
//            32 bits of its hash (4).  Slot and record together hold the whole hash, so growing the table (k_sd_rehash) walks the old slots
//            and reads the records only, never the arena;
//   arena    the strings' bytes, because the rows of earlier batches are gone.  Every string starts on a 16-byte boundary and is padded with
//            zero bytes to a multiple of 16: the compare (se_same_as) fetches the held string as aligned 16-byte words, ceil(len / 16) of
//            them when the string is aligned and ceil((skip + len) / 16) when it starts `skip` bytes into a word — for a 29-byte pod name 2
//            load instructions against 2.75 on average over the 16 starts.  What the compare costs is the number of load
//            instructions (the se_same_as comment), so the arena pays 7.5 bytes a value on average for the shorter compare.  The allocation's
//            length is a multiple of 16: every aligned 16-byte load of a compare stays inside it.
// One batch (tad_strdict_encode):
//   1. k_sd_probe: a workgroup takes 256 consecutive rows, stages their contiguous byte range in LDS with 16-byte loads (k_se_insert's rule:
//      kSeStage, per-lane global reads for a block over it or a lane outside the staged range), validates every span, hashes from LDS and
//      looks the string up.  Hit -> the code goes to the output; miss -> a flag byte, counted per wavefront.  The dictionary is only read.
//      A batch of known strings ends here: one pass, one synchronisation.
//   2. the misses are de-duplicated among themselves by launch_encode_strings with the miss flags as its keep mask: batch-local ids in
//      order of first appearance and the first row of each — deterministic, whatever order the wavefronts run in.  The local ids are
//      written to the miss rows of the output itself.
//   3. k_sd_lens + launch_scan: the new values' padded lengths become arena offsets (in 16-byte units, so that a count fits 32 bits).
//      The host reads the new-value count, the new bytes and the flags in one synchronisation and grows table, records or arena
//      into fresh allocations where needed (capacity only; the old arrays stay the dictionary's until the new ones are complete).
//   4. k_sd_append: one lane per NEW value copies the string from its first row into the arena in whole 8-byte words (se_load assembles
//      each word from aligned loads, whatever the source's alignment; the destination is 16-byte aligned), writes the record and claims a
//      slot.  New values are distinct from each other and from every value held, so nothing is compared here.
//   5. k_sd_fix: code = num_before + local id on the miss rows.
// The table never passes load 1/2 (grown BEFORE step 4), so every probe sequence ends at an empty slot and step 4 cannot fail.
// The other direction (tad_strdict_decode: arbitrary codes -> strings in Arrow's layout) reads records and arena only: k_sd_decode_lens,
// launch_scan, k_sd_decode — the staging of step 1 run backwards, the arena's alignment and padding doing for the reads what they do for
// the compare.
// Value masks read records and arena as well: k_sd_match (equality, the case-folded substring search) and k_sd_like (LIKE patterns with %
// and _: tad_like.h's token program in LDS), one lane per value.
// Retiring values (tad_strdict_compact): k_sd_compact_flags, two scans (new codes, new arena offsets), k_sd_compact_recs (remap and the new
// records), k_sd_compact_copy (the survivors' bytes, packed, in whole 16-byte words) and k_sd_compact_rehash (the old table's slots with
// their codes passed through remap) fill fresh records, a fresh arena and a fresh table; the host swaps them in last.
#include "tad_internal.h"
#include "tad_strbytes.h"

namespace tad {

static constexpr int kSdBlock = 256;

// record c: x = the string's byte offset in the arena, y = hash's low 32 bits << 32 | length
__device__ __forceinline__ uint32_t sd_rec_len(const ulonglong2 &r) { return (uint32_t)(r.y & 0xffffffffull); }
__device__ __forceinline__ uint32_t sd_rec_hash_lo(const ulonglong2 &r) { return (uint32_t)(r.y >> 32); }

// Step 1.  kInsert: a miss raises miss[v] (0 is written otherwise: the flags are the keep mask of step 2) and is counted; the code of a
// miss row is left to steps 2 and 5.  !kInsert (tad_strdict_lookup): a miss is TAD_CODE_NONE.  A word whose code is >= K is never a match
// (no such word exists in a dictionary that every call left normally).  A row whose offsets are unusable raises SD_FLAG_BAD_OFFSETS,
// reads no byte and is neither a hit nor a miss: the host fails the call.
template <bool kInsert>
__global__ __launch_bounds__(kSdBlock) void k_sd_probe(StrBatch A, const unsigned long long *__restrict__ table, uint64_t mask, const ulonglong2 *__restrict__ recs,
                                                       const uint8_t *__restrict__ arena, uint64_t K, long long *__restrict__ codes, uint8_t *__restrict__ miss,
                                                       unsigned long long *__restrict__ n_miss, uint32_t *__restrict__ flags) {
  __shared__ __attribute__((aligned(16))) uint64_t s_bytes[kSeStage / 8 + 4];
  __shared__ uint64_t s_lo, s_hi;
  uint32_t missed = 0;
  const uint32_t tid = threadIdx.x;
  for (uint64_t base = (uint64_t)blockIdx.x * kSdBlock; base < A.n; base += (uint64_t)gridDim.x * kSdBlock) {
    const uint64_t v = base + tid;
    const uint32_t rows = A.n - base < kSdBlock ? (uint32_t)(A.n - base) : kSdBlock;
    uint64_t b = 0; uint32_t len = 0;
    bool ok = true;
    if (tid < rows) ok = se_span(A, v, b, len);
    if (tid == 0) {
      // the block's byte range from its first and last row's RAW offsets (a null row reads as "" but its bytes may still be there)
      uint64_t lo, hi;
      if (A.off64) { const long long *o = static_cast<const long long *>(A.off); lo = (uint64_t)o[base]; hi = (uint64_t)o[base + rows]; }
      else { const int *o = static_cast<const int *>(A.off); lo = (uint64_t)(uint32_t)o[base]; hi = (uint64_t)(uint32_t)o[base + rows]; }
      s_lo = lo; s_hi = hi;
    }
    if (!ok) atomicOr(flags, SD_FLAG_BAD_OFFSETS);      // (the host fails the call; this lane skips its row)
    __syncthreads();                                    // (also: the previous round's strings are no longer read)
    const uint64_t lo = s_lo, hi = s_hi;
    const bool bad_range = hi < lo || hi > A.data_bytes;
    if (bad_range && tid == 0) atomicOr(flags, SD_FLAG_BAD_OFFSETS);
    const uintptr_t abs_lo = reinterpret_cast<uintptr_t>(A.data) + lo;
    const uintptr_t abs_a = abs_lo & ~(uintptr_t)15;    // the aligned 16-byte word that holds the range's first byte
    const uint64_t span = !bad_range && hi > lo ? (reinterpret_cast<uintptr_t>(A.data) + hi) - abs_a : 0;
    const bool block_staged = !bad_range && span <= kSeStage;     // block-uniform (from the shared bounds)
    if (block_staged && span) {
      const uint4 *src = reinterpret_cast<const uint4 *>(abs_a);
      uint4 *dst = reinterpret_cast<uint4 *>(s_bytes);
      for (uint32_t i = tid; (uint64_t)i * 16 < span; i += kSdBlock) dst[i] = src[i];   // (the last word may reach past `hi`: same aligned 16 bytes, same page)
    }
    __syncthreads();
    // a lane reads its string from the stage when it lies inside the staged range (always, for monotone offsets), else from global memory
    const bool staged = block_staged && b >= lo && b + len <= hi;
    if (tid < rows) {
      long long code = TAD_CODE_NONE;
      bool m = false;
      if (ok) {
        const uint8_t *p = A.data + b;
        const uint32_t at = staged ? (uint32_t)((reinterpret_cast<uintptr_t>(A.data) + b) - abs_a) : 0u;      // own string's offset in the stage
        uint64_t h = 0x9E3779B97F4A7C15ull ^ len;
        if (staged) {
          for (uint32_t i = 0; i < len; i += 8) h = fz_mix(h ^ se_load_lds(s_bytes, at + i, len - i < 8 ? len - i : 8)) + 0x632BE59BD9B4E019ull;
          h = fz_mix(h);
        } else {
          h = se_hash(p, len);
        }
        uint64_t held;
        m = !slot_find(table, mask, h, K, held, [&](uint64_t cand) {
          const ulonglong2 r = recs[cand];
          if (sd_rec_len(r) != len) return false;                   // lengths first
          const uint8_t *q = arena + r.x;
          return staged ? se_same_as([&](uint32_t o, uint32_t mm) { return se_load_lds(s_bytes, at + o, mm); }, q, len) : se_same(p, q, len);
        });
        if (!m) code = (long long)held;
      }
      if (kInsert) {
        miss[v] = m ? 1 : 0;
        missed += m ? 1u : 0u;
        if (!m) codes[v] = code;
      } else {
        codes[v] = code;
      }
    }
  }
  if (kInsert) wave_count_add(n_miss, missed);
}

// Step 3: cnt[j] = the 16-byte units new value j takes in the arena, for j < *num_new (step 2's count, on the device); 0 for the rest of
// the M entries the scan runs over, and for all of them when step 2 gave up (its flags: the host repeats it with a larger scratch table).
__global__ __launch_bounds__(kSdBlock) void k_sd_lens(StrBatch A, const uint64_t *__restrict__ first_row, const unsigned long long *__restrict__ num_new, uint64_t M,
                                                      const uint32_t *__restrict__ se_flags, uint32_t *__restrict__ cnt) {
  const uint64_t m = *se_flags != 0u ? 0ull : *num_new;
  for (uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; j < M; j += (uint64_t)gridDim.x * kSdBlock) {
    uint32_t units = 0;
    if (j < m) {
      const uint64_t v = first_row[j];
      uint64_t b; uint32_t len;
      if (v < A.n && se_span(A, v, b, len)) units = (uint32_t)(((uint64_t)len + 15) >> 4);
    }
    cnt[j] = units;
  }
}

// Step 4: one lane per new value.  first_row[j] = the row where new value j first appears (step 2), off16[j] = its place in the arena in
// 16-byte units behind arena_used (step 3).  The string is hashed while it is copied.  flags |= SD_FLAG_CLUSTER when a claim needed a long
// probe sequence: the host then grows the table after the call (a hint for speed; the claim itself always succeeds).
__global__ __launch_bounds__(kSdBlock) void k_sd_append(StrBatch A, const uint64_t *__restrict__ first_row, const unsigned long long *__restrict__ off16, uint64_t m,
                                                        uint64_t K0, uint64_t arena_used, unsigned long long *__restrict__ table, uint64_t mask,
                                                        ulonglong2 *__restrict__ recs, uint8_t *__restrict__ arena, uint32_t *__restrict__ flags) {
  for (uint64_t j = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kSdBlock) {
    const uint64_t v = first_row[j];
    uint64_t b; uint32_t len;
    if (v >= A.n || !se_span(A, v, b, len)) { atomicOr(flags, SD_FLAG_BAD_ROW); continue; }      // (cannot happen: steps 1 and 2 validated it)
    const uint64_t at = arena_used + off16[j] * 16ull;
    const uint8_t *p = A.data + b;
    uint64_t *dst = reinterpret_cast<uint64_t *>(arena + at);      // 16-byte aligned
    uint64_t h = 0x9E3779B97F4A7C15ull ^ len;
    for (uint32_t i = 0; i < len; i += 8) {
      const uint64_t x = se_load(p + i, len - i < 8 ? len - i : 8);     // bytes beyond the string are zero: the pad
      h = fz_mix(h ^ x) + 0x632BE59BD9B4E019ull;
      dst[i >> 3] = x;
    }
    if (((len + 7u) >> 3) & 1u) dst[(len + 7u) >> 3] = 0ull;            // the second half of the last 16 bytes
    h = fz_mix(h);
    recs[K0 + j] = ulonglong2{at, ((h & 0xffffffffull) << 32) | len};
    if (slot_claim(table, mask, h, slot_word(h, K0 + j)) > kSdMaxProbe) atomicOr(flags, SD_FLAG_CLUSTER);       // (K0 + j < 2^32 - 1: never the empty word)
  }
}

// Step 5 (the miss rows hold step 2's local ids)
__global__ __launch_bounds__(kSdBlock) void k_sd_fix(const uint8_t *__restrict__ miss, uint64_t n, uint64_t K0, long long *__restrict__ codes) {
  for (uint64_t v = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kSdBlock)
    if (miss[v] != 0) codes[v] += (long long)K0;
}

// The claimed slots of the old table into an EMPTY larger one (growth).  The slot gives the high half of the hash and the code, the code's
// record the low half: no string is read.
__global__ __launch_bounds__(kSdBlock) void k_sd_rehash(const unsigned long long *__restrict__ old_table, uint64_t old_slots, const ulonglong2 *__restrict__ recs, uint64_t K,
                                                        unsigned long long *__restrict__ table, uint64_t mask) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * kSdBlock) {
    const unsigned long long w = old_table[i];
    if (w == kSlotEmpty || (w & 0xffffffffull) >= K) continue;
    slot_claim(table, mask, ((w >> 32) << 32) | sd_rec_hash_lo(recs[w & 0xffffffffull]), w);
  }
}

// 'A'..'Z' -> 'a'..'z' in each of the eight bytes of x, every other byte — a byte >= 0x80 included — as it is
__device__ __forceinline__ uint64_t sd_fold(uint64_t x) {
  const uint64_t lo7 = x & 0x7f7f7f7f7f7f7f7full;
  const uint64_t ge_A = lo7 + 0x3f3f3f3f3f3f3f3full;      // bit 7 of a byte: its low seven bits are >= 0x41
  const uint64_t gt_Z = lo7 + 0x2525252525252525ull;      // ... are >= 0x5b
  return x | ((ge_A & ~gt_Z & ~x & 0x8080808080808080ull) >> 2);
}

// tad_strdict_match: one lane per value.  The pattern (already folded by the host for TAD_STR_CONTAINS_NOCASE) lies in LDS.  TAD_STR_EQUAL: the
// length, then the aligned 16-byte compare.  TAD_STR_CONTAINS_NOCASE: a plain search — for every start the value's bytes are taken as 8-byte
// words from ALIGNED 8-byte loads (the two words under the start stay in registers while the start moves through them), folded and compared with
// the pattern's words.  The matches are counted with one atomic per workgroup.
__global__ __launch_bounds__(kSdBlock) void k_sd_match(const ulonglong2 *__restrict__ recs, const uint8_t *__restrict__ arena, uint64_t K, int op,
                                                       const uint8_t *__restrict__ pattern, uint32_t plen, uint8_t *__restrict__ out, unsigned long long *__restrict__ n_hit) {
  __shared__ __attribute__((aligned(16))) uint64_t s_pat[kSdMaxPattern / 8 + 2];
  __shared__ uint32_t s_cnt[kSdBlock / 64];
  for (uint32_t i = threadIdx.x; i < kSdMaxPattern / 8 + 2; i += kSdBlock) s_pat[i] = 0ull;
  __syncthreads();
  uint8_t *pb = reinterpret_cast<uint8_t *>(s_pat);
  for (uint32_t i = threadIdx.x; i < plen; i += kSdBlock) pb[i] = pattern[i];
  __syncthreads();
  uint32_t mine = 0;
  const uint64_t first = plen ? se_load_lds(s_pat, 0, plen < 8 ? plen : 8) : 0ull;
  for (uint64_t c = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; c < K; c += (uint64_t)gridDim.x * kSdBlock) {
    const ulonglong2 r = recs[c];
    const uint32_t len = sd_rec_len(r);
    const uint8_t *q = arena + r.x;
    bool hit;
    if (op == TAD_STR_EQUAL) {
      hit = len == plen && se_same_as([&](uint32_t o, uint32_t m) { return se_load_lds(s_pat, o, m); }, q, len);
    } else if (plen == 0) {
      hit = true;
    } else if (len < plen) {
      hit = false;
    } else {
      hit = false;
      const uint64_t *w = reinterpret_cast<const uint64_t *>(q);      // 16-byte aligned, zero-padded to a multiple of 16
      const uint32_t m0 = plen < 8 ? plen : 8;
      const uint64_t keep0 = m0 < 8 ? (1ull << (m0 * 8)) - 1ull : ~0ull;
      uint64_t cur = w[0], nxt = len > 8 ? w[1] : 0ull;
      for (uint32_t i = 0; i + plen <= len && !hit; ++i) {
        const uint32_t sk = i & 7u;
        if (sk == 0 && i) { cur = nxt; nxt = i + 8 < len ? w[(i >> 3) + 1] : 0ull; }
        uint64_t x = cur >> (sk * 8);
        if (sk) x |= nxt << ((8 - sk) * 8);
        if (sd_fold(x & keep0) != first) continue;
        bool same = true;
        for (uint32_t k = 8; k < plen && same; k += 8) {
          const uint32_t m = plen - k < 8 ? plen - k : 8;
          same = sd_fold(se_load(q + i + k, m)) == se_load_lds(s_pat, k, m);
        }
        hit = same;
      }
    }
    out[c] = hit ? 1 : 0;
    mine += hit ? 1u : 0u;
  }
  block_count_add(s_cnt, n_hit, mine);
}

// tad_strdict_like: one lane per value, k_sd_match's shape.  The token program (tad_like.h: like_compile on the host) lies in LDS, two bytes a
// token; like_match walks it against the value.  The value's bytes come from ALIGNED 16-byte loads of the arena — every value starts on a
// 16-byte boundary and is padded to a multiple of 16, so the word that holds byte i < len lies inside the allocation — and the word under the
// cursor stays in two registers: the matcher moves forward a byte at a time and falls back to the last % only, so a word is loaded once per
// pass over it.  A value shorter than the program's least length is answered from its record.  No per-lane array: the byte is shifted out of
// the held word.  The matches are counted with one atomic per workgroup.
__global__ __launch_bounds__(kSdBlock) void k_sd_like(const ulonglong2 *__restrict__ recs, const uint8_t *__restrict__ arena, uint64_t K,
                                                      const uint16_t *__restrict__ prog, uint32_t n_tok, uint32_t min_len, uint32_t nocase,
                                                      uint8_t *__restrict__ out, unsigned long long *__restrict__ n_hit) {
  __shared__ uint16_t s_tok[kLikeMaxTokens];
  __shared__ uint32_t s_cnt[kSdBlock / 64];
  for (uint32_t i = threadIdx.x; i < n_tok && i < kLikeMaxTokens; i += kSdBlock) s_tok[i] = prog[i];
  __syncthreads();
  uint32_t mine = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; c < K; c += (uint64_t)gridDim.x * kSdBlock) {
    const ulonglong2 r = recs[c];
    const uint32_t len = sd_rec_len(r);
    bool hit = false;
    if (len >= min_len) {
      const ulonglong2 *w = reinterpret_cast<const ulonglong2 *>(arena + r.x);      // 16-byte aligned, zero-padded to a multiple of 16
      uint64_t lo = 0ull, hi = 0ull;                                                // the two halves of the 16-byte word held ...
      uint32_t at = ~0u;                                                            // ... and which one it is (none yet)
      auto byte = [&](uint32_t i) -> uint32_t {                                     // i < len
        if ((i >> 4) != at) {
          const ulonglong2 v = w[i >> 4];
          at = i >> 4; lo = v.x; hi = v.y;
        }
        const uint64_t a = lo, b = hi;                                              // (both read as values: a choice between two addresses would put them in memory)
        return (uint32_t)(((i & 8u) ? b : a) >> ((i & 7u) * 8u)) & 0xffu;
      };
      hit = like_match([&](uint32_t p) -> uint32_t { return s_tok[p]; }, n_tok, byte, len, nocase != 0u);
    }
    out[c] = hit ? 1 : 0;
    mine += hit ? 1u : 0u;
  }
  block_count_add(s_cnt, n_hit, mine);
}

// tad_strdict_export: cnt[i] = the length of value first + i (the scan of it gives Arrow's offsets) ...
__global__ __launch_bounds__(kSdBlock) void k_sd_export_lens(const ulonglong2 *__restrict__ recs, uint64_t first, uint64_t n, uint32_t *__restrict__ cnt) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSdBlock) cnt[i] = sd_rec_len(recs[first + i]);
}

// ... and the bytes packed behind each other: one lane per value; single bytes up to the destination's next 8-byte boundary, whole words from
// there (se_load: the source is then misaligned by whatever the head took), single bytes for the tail.  `out` is 8-byte aligned.
__global__ __launch_bounds__(kSdBlock) void k_sd_export(const ulonglong2 *__restrict__ recs, const uint8_t *__restrict__ arena, uint64_t first, uint64_t n,
                                                        const unsigned long long *__restrict__ off, uint8_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSdBlock) {
    const ulonglong2 r = recs[first + i];
    const uint32_t len = sd_rec_len(r);
    const uint8_t *q = arena + r.x;
    uint8_t *d = out + off[i];
    uint32_t k = 0;
    const uint32_t head = (uint32_t)((8u - (uint32_t)(off[i] & 7ull)) & 7u);
    for (; k < len && k < head; ++k) d[k] = q[k];
    for (; k + 8 <= len; k += 8) *reinterpret_cast<uint64_t *>(d + k) = se_load(q + k, 8);
    for (; k < len; ++k) d[k] = q[k];
  }
}

// ---- tad_strdict_decode: codes -> strings ----
// Lengths: cnt[i] = the length of value codes[i], read from its record (one 16-byte load a row).  A code outside [0, K) — TAD_CODE_NONE is
// one — counts 0 and raises SD_FLAG_BAD_CODE: the host refuses the call before a byte is copied.
__global__ __launch_bounds__(kSdBlock) void k_sd_decode_lens(const ulonglong2 *__restrict__ recs, uint64_t K, const long long *__restrict__ codes, uint64_t n,
                                                             uint32_t *__restrict__ cnt, uint32_t *__restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSdBlock) {
    const uint64_t c = (uint64_t)codes[i];      // (a negative code is a huge unsigned one)
    const bool in = c < K;
    if (!in) atomicOr(flags, SD_FLAG_BAD_CODE);
    cnt[i] = in ? sd_rec_len(recs[c]) : 0u;
  }
}

// 8-byte word k of a held string of len bytes with the bytes at and beyond len zeroed (they are the arena's pad: zero as k_sd_append left
// them, but nothing of a pad may reach the output whatever it holds)
__device__ __forceinline__ uint64_t sd_keep(uint64_t x, uint64_t k, uint64_t len) {
  const uint64_t b = k * 8;
  if (b + 8 <= len) return x;
  return b >= len ? 0ull : x & ((1ull << ((len - b) * 8)) - 1ull);
}

// A held string q (16-byte aligned in the arena, padded to a multiple of 16) as the ALIGNED 8-byte words of a destination in which it
// begins s (0..7) bytes into word 0: put(k, x) for the words k = 2 j, 2 j + 1 of j = j0, j0 + step, ... — x holds the string's bytes
// [8 k - s, 8 k - s + 8) in place and zeros elsewhere.  Every source read is an aligned 16-byte load inside the allocation, but for the
// 8 bytes in front of a pair when another lane loaded them (step > 1): one more aligned 8-byte load of the line just read.
template <class Put>
__device__ __forceinline__ void sd_shifted_words(const uint8_t *q, uint64_t len, uint32_t s, uint64_t j0, uint64_t step, Put put) {
  const ulonglong2 *q16 = reinterpret_cast<const ulonglong2 *>(q);
  const uint64_t *q64 = reinterpret_cast<const uint64_t *>(q);
  const uint64_t nw16 = (len + 15) >> 4, ndw = (s + len + 7) >> 3;
  const uint32_t sh = s * 8u;
  uint64_t carried = 0;
  for (uint64_t j = j0; 2 * j < ndw; j += step) {
    const ulonglong2 v = j < nw16 ? q16[j] : ulonglong2{0ull, 0ull};      // (j == nw16: the word that takes the last bytes shifted out)
    const uint64_t a = sd_keep(v.x, 2 * j, len), b = sd_keep(v.y, 2 * j + 1, len);
    uint64_t prev = 0;
    if (sh != 0u && j != 0) prev = (step == 1 && j != j0) ? carried : sd_keep(q64[2 * j - 1], 2 * j - 1, len);
    put(2 * j, sh ? (a << sh) | (prev >> (64u - sh)) : a);
    if (2 * j + 1 < ndw) put(2 * j + 1, sh ? (b << sh) | (a >> (64u - sh)) : b);
    carried = b;
  }
}

static constexpr uint32_t kSdDecodeLaneMax = 128;      // a longer string of a staged tile is assembled by a wavefront, not by its row's lane

#ifndef TAD_SD_DECODE_ROWS
// Copy, the shipped form: k_sd_probe's staging run backwards.  A workgroup takes kSdDecodeRows consecutive rows; their output bytes
// [off[r0], off[r1]) are contiguous.  A tile of at most kSdDecodeStage bytes is assembled in LDS, laid out as the 16-byte words of the
// DESTINATION (the tile begins `head` = its address mod 16 bytes into word 0): the stage is zeroed, every lane ORs its row's shifted words
// into it (rows share the words at their ends, and never a byte), a row over kSdDecodeLaneMax bytes is left to a wavefront.  The stage then
// goes out in aligned 16-byte stores, consecutive lanes on consecutive words: the output crosses the memory system once, in whole lines.
// Only the bytes of the partial words at the tile's two ends are stored singly — the neighbouring tiles own the rest of those words.
// A tile over the stage (long labels, one long string) is not staged: its rows are taken in turn by the wavefronts, 64 lanes on
// consecutive 8-byte words of the destination, single bytes where a word is shared with the next row.
__global__ __launch_bounds__(kSdBlock) void k_sd_decode(const ulonglong2 *__restrict__ recs, const uint8_t *__restrict__ arena, const long long *__restrict__ codes,
                                                        uint64_t n, const unsigned long long *__restrict__ off, uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_stage[kSdDecodeStage / 8 + 4];      // (+ 16: head, + 16: the last word's other half)
  __shared__ uint16_t s_long[kSdDecodeRows];
  __shared__ uint32_t s_nlong;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * kSdDecodeRows; base < n; base += (uint64_t)gridDim.x * kSdDecodeRows) {
    const uint32_t rows = n - base < kSdDecodeRows ? (uint32_t)(n - base) : kSdDecodeRows;
    const uint64_t lo = off[base], total = off[base + rows] - lo;      // block-uniform
    if (total == 0) continue;
    if (total <= kSdDecodeStage) {
      const uint32_t head = (uint32_t)(reinterpret_cast<uintptr_t>(out + lo) & 15u), end = head + (uint32_t)total;
      uint4 *stage16 = reinterpret_cast<uint4 *>(s_stage);
      if (tid == 0) s_nlong = 0;
      for (uint32_t i = tid; i < (end + 15u) >> 4; i += kSdBlock) stage16[i] = uint4{0u, 0u, 0u, 0u};
      __syncthreads();
      if (tid < rows) {
        const ulonglong2 r = recs[codes[base + tid]];
        const uint32_t len = sd_rec_len(r);
        if (len > kSdDecodeLaneMax) {
          s_long[atomicAdd(&s_nlong, 1u)] = (uint16_t)tid;
        } else if (len != 0u) {
          const uint32_t at = head + (uint32_t)(off[base + tid] - lo);
          sd_shifted_words(arena + r.x, len, at & 7u, 0, 1, [&](uint64_t k, uint64_t x) { atomicOr(&s_stage[(at >> 3) + k], (unsigned long long)x); });
        }
      }
      __syncthreads();
      const uint32_t nlong = s_nlong;
      for (uint32_t i = wave; i < nlong; i += kSdBlock / 64) {
        const uint32_t t = s_long[i];
        const ulonglong2 r = recs[codes[base + t]];
        const uint32_t at = head + (uint32_t)(off[base + t] - lo);
        sd_shifted_words(arena + r.x, sd_rec_len(r), at & 7u, lane, 64, [&](uint64_t k, uint64_t x) { atomicOr(&s_stage[(at >> 3) + k], (unsigned long long)x); });
      }
      if (nlong != 0u) __syncthreads();
      uint8_t *dst = out + lo - head;                           // 16-byte aligned; the stage's byte p belongs at dst + p, for head <= p < end
      const uint32_t first = head != 0u ? 1u : 0u, last = end >> 4;      // [first, last): the words that are the tile's alone
      for (uint32_t i = first + tid; i < last; i += kSdBlock) reinterpret_cast<uint4 *>(dst)[i] = stage16[i];
      const uint8_t *stage8 = reinterpret_cast<const uint8_t *>(s_stage);
      if (tid < 16u) {
        if (head != 0u && tid >= head && tid < end) dst[tid] = stage8[tid];
      } else if (tid < 32u) {
        const uint32_t p = last * 16u + (tid - 16u);
        if ((last != 0u || head == 0u) && p < end) dst[p] = stage8[p];
      }
      __syncthreads();                                          // (the next round zeroes the stage)
    } else {
      for (uint32_t t = wave; t < rows; t += kSdBlock / 64) {
        const ulonglong2 r = recs[codes[base + t]];
        const uint64_t len = sd_rec_len(r);
        if (len == 0) continue;
        uint8_t *d = out + off[base + t];
        const uint32_t s = (uint32_t)(reinterpret_cast<uintptr_t>(d) & 7u);
        uint8_t *d0 = d - s;                                    // 8-byte aligned
        sd_shifted_words(arena + r.x, len, s, lane, 64, [&](uint64_t k, uint64_t x) {
          const long long b0 = (long long)(k * 8) - (long long)s;      // the string's byte at the word's byte 0
          const uint32_t t0 = b0 < 0 ? (uint32_t)(-b0) : 0u, t1 = (long long)len - b0 < 8 ? (uint32_t)((long long)len - b0) : 8u;
          if (t0 == 0u && t1 == 8u) *reinterpret_cast<uint64_t *>(d0 + k * 8) = x;
          else for (uint32_t b = t0; b < t1; ++b) d0[k * 8 + b] = (uint8_t)(x >> (b * 8u));
        });
      }
    }
  }
}
#else
// Copy, the plain form (measured against the tiled one: DESIGN.md §5): k_sd_export's loop on gathered records — one lane per row, single
// bytes up to the destination's next 8-byte boundary, whole words from there, single bytes for the tail.
__global__ __launch_bounds__(kSdBlock) void k_sd_decode(const ulonglong2 *__restrict__ recs, const uint8_t *__restrict__ arena, const long long *__restrict__ codes,
                                                        uint64_t n, const unsigned long long *__restrict__ off, uint8_t *__restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSdBlock) {
    const ulonglong2 r = recs[codes[i]];
    const uint32_t len = sd_rec_len(r);
    const uint8_t *q = arena + r.x;
    uint8_t *d = out + off[i];
    uint32_t k = 0;
    const uint32_t head = (uint32_t)((8u - (uint32_t)(reinterpret_cast<uintptr_t>(d) & 7u)) & 7u);
    for (; k < len && k < head; ++k) d[k] = q[k];
    for (; k + 8 <= len; k += 8) *reinterpret_cast<uint64_t *>(d + k) = se_load(q + k, 8);
    for (; k < len; ++k) d[k] = q[k];
  }
}
#endif

// ---- tad_strdict_compact: retired values leave, the survivors are renumbered densely, the arena is packed ----
// Flags: live[c] = keep[c] != 0 and units[c] = the 16-byte units a survivor takes in the arena (0 for a retired value).  The scan of live
// gives the new codes, the scan of units the new arena offsets — in 16-byte units, so that a count fits 32 bits, as in step 3 of the encode.
__global__ __launch_bounds__(kSdBlock) void k_sd_compact_flags(const uint8_t *__restrict__ keep, const ulonglong2 *__restrict__ recs, uint64_t K, uint32_t *__restrict__ live,
                                                               uint32_t *__restrict__ units) {
  for (uint64_t c = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; c < K; c += (uint64_t)gridDim.x * kSdBlock) {
    const bool alive = keep[c] != 0;
    live[c] = alive ? 1u : 0u;
    units[c] = alive ? (uint32_t)(((uint64_t)sd_rec_len(recs[c]) + 15) >> 4) : 0u;
  }
}

// Records: one lane per OLD value writes remap[c] — the new code, TAD_CODE_NONE for a retired value.  kMove: a survivor also writes its new
// record (the new offset; length and low hash copied) and, by new code, where its bytes lie in the old arena (src16, in 16-byte units).
template <bool kMove>
__global__ __launch_bounds__(kSdBlock) void k_sd_compact_recs(const uint32_t *__restrict__ live, const unsigned long long *__restrict__ newcode,
                                                              const unsigned long long *__restrict__ off16, const ulonglong2 *__restrict__ recs, uint64_t K,
                                                              long long *__restrict__ remap, ulonglong2 *__restrict__ nrecs, unsigned long long *__restrict__ src16) {
  for (uint64_t c = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; c < K; c += (uint64_t)gridDim.x * kSdBlock) {
    const bool alive = live[c] != 0u;
    const unsigned long long j = newcode[c];
    remap[c] = alive ? (long long)j : (long long)TAD_CODE_NONE;
    if (kMove && alive) {
      const ulonglong2 r = recs[c];
      nrecs[j] = ulonglong2{off16[c] * 16ull, r.y};
      src16[j] = r.x >> 4;
    }
  }
}

// Arena copy.  Source and destination strings are both 16-byte aligned and zero-padded to a multiple of 16, so whole 16-byte words move and
// no byte is shifted.  A workgroup takes kSdBlock consecutive SURVIVORS: their destination range is contiguous (the new arena is packed), and
// their first destination words — relative to the tile's — and source words lie in LDS.  The lanes walk the destination's words in order,
// consecutive lanes on consecutive words; each finds its row by a search in the LDS offsets and loads the word from the old arena: aligned
// 16-byte stores in whole lines out, a gather in.  A survivor of more than kSdCopyLaneMax words (one workgroup pass) is stepped over by the walk
// and taken by the wavefronts in turn, 64 lanes on consecutive words, as k_sd_decode treats a tile over its stage.
static constexpr uint32_t kSdCopyLaneMax = kSdBlock;
__global__ __launch_bounds__(kSdBlock) void k_sd_compact_copy(const ulonglong2 *__restrict__ nrecs, const unsigned long long *__restrict__ src16, uint64_t m,
                                                              const uint8_t *__restrict__ arena, uint8_t *__restrict__ narena) {
  __shared__ unsigned long long s_dst[kSdBlock + 1];      // row r's first destination word; s_dst[rows] = the tile's words
  __shared__ unsigned long long s_src[kSdBlock];
  __shared__ uint16_t s_long[kSdBlock];
  __shared__ uint32_t s_nlong;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint4 *src = reinterpret_cast<const uint4 *>(arena);
  uint4 *dst = reinterpret_cast<uint4 *>(narena);
  for (uint64_t base = (uint64_t)blockIdx.x * kSdBlock; base < m; base += (uint64_t)gridDim.x * kSdBlock) {
    const uint32_t rows = m - base < kSdBlock ? (uint32_t)(m - base) : kSdBlock;
    const uint64_t tile0 = nrecs[base].x >> 4;            // block-uniform
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    if (tid < rows) {
      const ulonglong2 r = nrecs[base + tid];
      const uint64_t at = (r.x >> 4) - tile0, u = ((uint64_t)sd_rec_len(r) + 15) >> 4;
      s_dst[tid] = at;
      s_src[tid] = src16[base + tid];
      if (tid == rows - 1) s_dst[rows] = at + u;
      if (u > kSdCopyLaneMax) s_long[atomicAdd(&s_nlong, 1u)] = (uint16_t)tid;
    }
    __syncthreads();
    const uint64_t total = s_dst[rows];
    const uint32_t nlong = s_nlong;
    for (uint64_t w = tid; w < total; w += kSdBlock) {
      uint32_t lo = 0, hi = rows;                         // s_dst[lo] <= w < s_dst[hi]: rows of no bytes are passed over
      while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_dst[mid] <= w) lo = mid; else hi = mid;
      }
      const uint64_t first = s_dst[lo], end = s_dst[lo + 1];
      if (nlong != 0u && end - first > kSdCopyLaneMax) {      // a long row: on to this lane's first word behind it, without a search per word
        w += (end - w - 1) / kSdBlock * kSdBlock;
        continue;
      }
      dst[tile0 + w] = src[s_src[lo] + (w - first)];
    }
    for (uint32_t i = wave; i < nlong; i += kSdBlock / 64) {
      const uint32_t t = s_long[i];
      const uint64_t first = s_dst[t], n = s_dst[t + 1] - first, from = s_src[t];
      for (uint64_t k = lane; k < n; k += 64) dst[tile0 + first + k] = src[from + k];
    }
    __syncthreads();                                      // (the next round rewrites the offsets and the list)
  }
}

// Table: k_sd_rehash on the OLD table's claimed slots with the codes passed through remap.  The slot gives the high half of the hash and
// the old code, the old record the low half; a survivor claims fingerprint << 32 | remap[code] in the fresh table.  No string is read.
__global__ __launch_bounds__(kSdBlock) void k_sd_compact_rehash(const unsigned long long *__restrict__ old_table, uint64_t old_slots, const ulonglong2 *__restrict__ recs,
                                                                uint64_t K, const long long *__restrict__ remap, unsigned long long *__restrict__ table, uint64_t mask) {
  for (uint64_t i = (uint64_t)blockIdx.x * kSdBlock + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * kSdBlock) {
    const unsigned long long w = old_table[i];
    const uint64_t c = w & 0xffffffffull;
    if (w == kSlotEmpty || c >= K) continue;
    const long long j = remap[c];
    if (j < 0) continue;
    slot_claim(table, mask, ((w >> 32) << 32) | sd_rec_hash_lo(recs[c]), ((w >> 32) << 32) | (unsigned long long)j);
  }
}

static dim3 sd_grid(uint64_t items) { const uint64_t b = (items + kSdBlock - 1) / kSdBlock; return dim3((unsigned)(b < 16384 ? (b ? b : 1) : 16384)); }

void launch_sd_probe(hipStream_t s, const StrBatch &B, const unsigned long long *table, uint64_t slots, const void *recs, const uint8_t *arena, uint64_t K,
                     long long *codes, uint8_t *miss, unsigned long long *n_miss, uint32_t *flags) {
  const ulonglong2 *r = static_cast<const ulonglong2 *>(recs);
  if (miss != nullptr) hipLaunchKernelGGL(k_sd_probe<true>, sd_grid(B.n), dim3(kSdBlock), 0, s, B, table, slots - 1, r, arena, K, codes, miss, n_miss, flags);
  else hipLaunchKernelGGL(k_sd_probe<false>, sd_grid(B.n), dim3(kSdBlock), 0, s, B, table, slots - 1, r, arena, K, codes, miss, n_miss, flags);
}

void launch_sd_lens(hipStream_t s, const StrBatch &B, const uint64_t *first_row, const unsigned long long *num_new, uint64_t M, const uint32_t *se_flags, uint32_t *cnt) {
  hipLaunchKernelGGL(k_sd_lens, sd_grid(M), dim3(kSdBlock), 0, s, B, first_row, num_new, M, se_flags, cnt);
}

void launch_sd_append(hipStream_t s, const StrBatch &B, const uint64_t *first_row, const unsigned long long *off16, uint64_t m, uint64_t K0, uint64_t arena_used,
                      unsigned long long *table, uint64_t slots, void *recs, uint8_t *arena, uint32_t *flags) {
  hipLaunchKernelGGL(k_sd_append, sd_grid(m), dim3(kSdBlock), 0, s, B, first_row, off16, m, K0, arena_used, table, slots - 1, static_cast<ulonglong2 *>(recs), arena,
                     flags);
}

void launch_sd_fix(hipStream_t s, const uint8_t *miss, uint64_t n, uint64_t K0, long long *codes) {
  hipLaunchKernelGGL(k_sd_fix, sd_grid(n), dim3(kSdBlock), 0, s, miss, n, K0, codes);
}

void launch_sd_rehash(hipStream_t s, const unsigned long long *old_table, uint64_t old_slots, const void *recs, uint64_t K, unsigned long long *table, uint64_t slots) {
  hipLaunchKernelGGL(k_sd_rehash, sd_grid(old_slots), dim3(kSdBlock), 0, s, old_table, old_slots, static_cast<const ulonglong2 *>(recs), K, table, slots - 1);
}

void launch_sd_match(hipStream_t s, const void *recs, const uint8_t *arena, uint64_t K, int op, const uint8_t *pattern, uint32_t pattern_len, uint8_t *out,
                     unsigned long long *n_hit) {
  if (K == 0) return;
  hipLaunchKernelGGL(k_sd_match, sd_grid(K), dim3(kSdBlock), 0, s, static_cast<const ulonglong2 *>(recs), arena, K, op, pattern, pattern_len, out, n_hit);
}

void launch_sd_like(hipStream_t s, const void *recs, const uint8_t *arena, uint64_t K, const uint16_t *prog, uint32_t n_tok, uint32_t min_len, bool nocase,
                    uint8_t *out, unsigned long long *n_hit) {
  if (K == 0) return;
  const uint64_t b = (K + kSdBlock - 1) / kSdBlock;
  hipLaunchKernelGGL(k_sd_like, dim3((unsigned)(b < kSdLikeMaxBlocks ? b : kSdLikeMaxBlocks)), dim3(kSdBlock), 0, s, static_cast<const ulonglong2 *>(recs), arena, K,
                     prog, n_tok, min_len, nocase ? 1u : 0u, out, n_hit);
}

void launch_sd_export_lens(hipStream_t s, const void *recs, uint64_t first, uint64_t n, uint32_t *cnt) {
  hipLaunchKernelGGL(k_sd_export_lens, sd_grid(n), dim3(kSdBlock), 0, s, static_cast<const ulonglong2 *>(recs), first, n, cnt);
}

void launch_sd_export(hipStream_t s, const void *recs, const uint8_t *arena, uint64_t first, uint64_t n, const unsigned long long *off, uint8_t *out) {
  hipLaunchKernelGGL(k_sd_export, sd_grid(n), dim3(kSdBlock), 0, s, static_cast<const ulonglong2 *>(recs), arena, first, n, off, out);
}

void launch_sd_decode_lens(hipStream_t s, const void *recs, uint64_t K, const long long *codes, uint64_t n, uint32_t *cnt, uint32_t *flags) {
  hipLaunchKernelGGL(k_sd_decode_lens, sd_grid(n), dim3(kSdBlock), 0, s, static_cast<const ulonglong2 *>(recs), K, codes, n, cnt, flags);
}

void launch_sd_decode(hipStream_t s, const void *recs, const uint8_t *arena, const long long *codes, uint64_t n, const unsigned long long *off, uint8_t *out) {
  static_assert(kSdDecodeRows == kSdBlock, "a lane per row of the tile");
  const uint64_t tiles = (n + kSdDecodeRows - 1) / kSdDecodeRows;      // past kSdDecodeMaxBlocks workgroups the tiles are taken in a grid stride
  hipLaunchKernelGGL(k_sd_decode, dim3((unsigned)(tiles < kSdDecodeMaxBlocks ? (tiles ? tiles : 1) : kSdDecodeMaxBlocks)), dim3(kSdBlock), 0, s,
                     static_cast<const ulonglong2 *>(recs), arena, codes, n, off, out);
}

void launch_sd_compact_flags(hipStream_t s, const uint8_t *keep, const void *recs, uint64_t K, uint32_t *live, uint32_t *units) {
  hipLaunchKernelGGL(k_sd_compact_flags, sd_grid(K), dim3(kSdBlock), 0, s, keep, static_cast<const ulonglong2 *>(recs), K, live, units);
}

void launch_sd_compact_recs(hipStream_t s, const uint32_t *live, const unsigned long long *newcode, const unsigned long long *off16, const void *recs, uint64_t K,
                            long long *remap, void *nrecs, unsigned long long *src16) {
  const ulonglong2 *r = static_cast<const ulonglong2 *>(recs);
  if (nrecs != nullptr) hipLaunchKernelGGL(k_sd_compact_recs<true>, sd_grid(K), dim3(kSdBlock), 0, s, live, newcode, off16, r, K, remap, static_cast<ulonglong2 *>(nrecs), src16);
  else hipLaunchKernelGGL(k_sd_compact_recs<false>, sd_grid(K), dim3(kSdBlock), 0, s, live, newcode, off16, r, K, remap, static_cast<ulonglong2 *>(nullptr), src16);
}

void launch_sd_compact_copy(hipStream_t s, const void *nrecs, const unsigned long long *src16, uint64_t m, const uint8_t *arena, uint8_t *narena) {
  if (m == 0) return;
  const uint64_t tiles = (m + kSdBlock - 1) / kSdBlock;      // past kSdDecodeMaxBlocks workgroups the tiles are taken in a grid stride
  hipLaunchKernelGGL(k_sd_compact_copy, dim3((unsigned)(tiles < kSdDecodeMaxBlocks ? tiles : kSdDecodeMaxBlocks)), dim3(kSdBlock), 0, s,
                     static_cast<const ulonglong2 *>(nrecs), src16, m, arena, narena);
}

void launch_sd_compact_rehash(hipStream_t s, const unsigned long long *old_table, uint64_t old_slots, const void *recs, uint64_t K, const long long *remap,
                              unsigned long long *table, uint64_t slots) {
  hipLaunchKernelGGL(k_sd_compact_rehash, sd_grid(old_slots), dim3(kSdBlock), 0, s, old_table, old_slots, static_cast<const ulonglong2 *>(recs), K, remap, table, slots - 1);
}

// one kernel of this translation unit: tad_engine_create resolves it so that the unit's code object is loaded before the first batch
const void *code_anchor_strdict() { return reinterpret_cast<const void *>(&k_sd_fix); }

}  // namespace tad
