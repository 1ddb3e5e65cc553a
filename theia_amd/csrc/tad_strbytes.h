// tad_strbytes.h — the byte helpers of the string kernels: a row's span in an Arrow string column (StrBatch, tad_internal.h), its bytes as
// little-endian words from global memory and from an LDS stage, the hash and the aligned 16-byte compare.  Shared by tad_factorize.hip
// (tad_encode_strings: the strings of one call) and tad_strdict.hip (tad_strdict: the strings of every call); device code only, included by
// those two files.
#pragma once
#include "tad_internal.h"
#include "tad_slots.h"      // fz_mix, and the slot table for both includers

namespace tad {

// [b, b + len) of row v; false if the offsets are not usable
__device__ __forceinline__ bool se_span(const StrBatch &A, uint64_t v, uint64_t &b, uint32_t &len) {
  uint64_t e;
  if (A.off64) {
    const long long *o = static_cast<const long long *>(A.off);
    b = (uint64_t)o[v]; e = (uint64_t)o[v + 1];
  } else {
    const int *o = static_cast<const int *>(A.off);
    b = (uint64_t)(uint32_t)o[v]; e = (uint64_t)(uint32_t)o[v + 1];
  }
  if (e < b || e > A.data_bytes || e - b > 0xFFFFFFFFull) return false;
  len = (uint32_t)(e - b);
  if (A.valid != nullptr) {
    const uint64_t bit = A.valid_off + v;
    if (((A.valid[bit >> 3] >> (bit & 7)) & 1u) == 0) len = 0;   // null = ""
  }
  return true;
}

// m (1..8) bytes at p as a little-endian word, bytes beyond m zero.  Two aligned loads without a branch between them (a conditional second load
// made every chunk of a compare its own memory round trip): when the chunk does not reach into the next word, the first word is loaded twice.
__device__ __forceinline__ uint64_t se_load(const uint8_t *p, uint32_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint64_t *w = reinterpret_cast<const uint64_t *>(a & ~(uintptr_t)7);
  const uint32_t skip = (uint32_t)(a & 7);           // bytes of w[0] in front of p
  const bool two = skip + m > 8;                      // (skip >= 1 then: the left shift below is < 64)
  const uint64_t lo = w[0], hi = w[two ? 1 : 0];
  uint64_t x = lo >> (skip * 8);
  if (two) x |= hi << ((8 - skip) * 8);
  if (m < 8) x &= (1ull << (m * 8)) - 1ull;
  return x;
}

__device__ __forceinline__ uint64_t se_hash(const uint8_t *p, uint32_t len) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ len;
  for (uint32_t i = 0; i < len; i += 8) h = fz_mix(h ^ se_load(p + i, len - i < 8 ? len - i : 8)) + 0x632BE59BD9B4E019ull;
  return fz_mix(h);
}

// own(at, m): m bytes of the lane's own string at offset `at`; q: the representative row's bytes in global memory.  What the compare costs is
// the number of load instructions — 64 lanes, 64 different representatives, 64 different cache lines per instruction, all from L2 — not their
// latency (3.4 of the insert pass's 5.1 ms, profiles/r4_v33_*; loading the chunks four at a time changed nothing).  So the representative's bytes
// are fetched as ALIGNED 16-byte words, each exactly once (a 29-byte name is 2-3 loads; chunk by chunk through se_load it was 8: every aligned word
// twice), and each 8-byte half is compared with the bytes of the own string it covers.
template <class Own>
__device__ __forceinline__ bool se_same_as(Own own, const uint8_t *q, uint32_t len) {
  if (len == 0) return true;                               // (nothing to read: the lengths are equal)
  const uintptr_t a = reinterpret_cast<uintptr_t>(q);
  const ulonglong2 *w = reinterpret_cast<const ulonglong2 *>(a & ~(uintptr_t)15);
  const int skip = (int)(a & 15);                          // bytes of w[0] in front of the string
  const uint32_t nw = ((uint32_t)skip + len + 15u) >> 4;   // aligned 16-byte words that hold a byte of the string (each inside the buffer's pages)
  bool same = true;
  for (uint32_t k0 = 0; k0 < nw && same; k0 += 2) {
    ulonglong2 v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) v[u] = w[k0 + u < nw ? k0 + u : k0];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (k0 + u >= nw) break;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int start = (int)(16u * (k0 + u)) + 8 * h - skip;        // offset in the string of this 8-byte half's first byte (may be < 0)
        const int s0 = start < 0 ? 0 : start;
        const int e0 = start + 8 < (int)len ? start + 8 : (int)len;
        if (e0 <= s0) continue;                                         // the half lies before or behind the string
        const uint32_t m = (uint32_t)(e0 - s0);
        uint64_t x = (h == 0 ? v[u].x : v[u].y) >> (8 * (s0 - start));
        if (m < 8) x &= (1ull << (m * 8)) - 1ull;
        same = same && x == own((uint32_t)s0, m);
      }
    }
  }
  return same;
}
__device__ __forceinline__ bool se_same(const uint8_t *p, const uint8_t *q, uint32_t len) {
  return se_same_as([&](uint32_t at, uint32_t m) { return se_load(p + at, m); }, q, len);
}

// A block's rows are CONSECUTIVE rows of the column, so their bytes are one contiguous range [off[r0], off[r0 + 256)) of `data`: it is copied
// into LDS with 16-byte loads (consecutive lanes on consecutive 16 bytes: the column's bytes cross the memory system once, in whole lines),
// and every lane then hashes and compares its own string from LDS.  Per-lane 8-byte global loads at a ~29-byte stride — the first version —
// made every wave-level load touch ~15 cache lines, five times over per row, and ran at 0.07 of the HBM peak (profiles/r4_v28_*).
// A block whose 256 rows hold more than kSeStage bytes (long labels) reads its strings from global memory lane by lane instead.
static constexpr uint32_t kSeStage = 24 * 1024;

// m (1..8) bytes at byte offset `at` of an 8-byte aligned LDS buffer, bytes beyond m zero
__device__ __forceinline__ uint64_t se_load_lds(const uint64_t *buf, uint32_t at, uint32_t m) {
  const uint32_t skip = at & 7u;
  uint64_t x = buf[at >> 3] >> (skip * 8);
  if (skip + m > 8) x |= buf[(at >> 3) + 1] << ((8 - skip) * 8);
  if (m < 8) x &= (1ull << (m * 8)) - 1ull;
  return x;
}

}  // namespace tad
