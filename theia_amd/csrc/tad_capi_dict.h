// tad_capi_dict.h — what the host sides of the four ingest encoders share (tad_capi_ingest.cpp: tad_factorize, tad_encode_strings;
// tad_capi_keydict.cpp; tad_capi_strdict.cpp): candidate device arrays that free themselves, the growth of a slot table, the table-size
// ladder of tad_factorize.hip and the staging of a host batch into device scratch.  Header only: every body is a template or small.
#ifndef THEIA_TAD_CAPI_DICT_H
#define THEIA_TAD_CAPI_DICT_H

#include "tad_engine.h"

namespace tadh {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
inline uint64_t pow2_at_least(uint64_t x) { uint64_t s = 64; while (s < x) s <<= 1; return s; }   // a dictionary's table: 64 slots at least

// A candidate device array: filled beside the array it may replace, which stays the dictionary's until commit_into — so a call that leaves
// early, on whatever path, leaves the dictionary as it was and nothing behind.  cap: the capacity in the owner's units.
template <typename T> struct Candidate {
  T *p = nullptr;
  uint64_t cap = 0;
  Candidate() = default;
  Candidate(const Candidate &) = delete;
  Candidate &operator=(const Candidate &) = delete;
  ~Candidate() { if (p) hipFree(p); }
  hipError_t alloc(JobCtx *e, uint64_t cap_, size_t bytes) {
    cap = cap_;
    return dev_alloc(e, reinterpret_cast<void **>(&p), bytes);
  }
  // the old array goes, this one takes its place (nothing allocated: nothing happens)
  template <typename U> void commit_into(U *&old_ptr, uint64_t &old_cap) {
    if (!p) return;
    hipFree(old_ptr);
    old_ptr = static_cast<U *>(p);
    old_cap = cap;
    p = nullptr;
  }
};

// A larger slot table for a dictionary of `total` keys: load <= 1/2, at least min_slots, never smaller than the `slots` it has.  Nothing to
// grow: nt stays empty.  Else nt = a fresh table, cleared to all ones, and rehash(nt->p, nt->cap) puts the dictionary's keys on the stream.
template <class Rehash>
hipError_t grow_table(JobCtx *e, uint64_t slots, uint64_t total, uint64_t min_slots, Candidate<unsigned long long> *nt, Rehash rehash) {
  uint64_t nslots = 2 * total > slots ? pow2_at_least(2 * total) : slots;
  if (min_slots > nslots) nslots = min_slots;
  if (nslots == slots) return hipSuccess;
  hipError_t r = nt->alloc(e, nslots, nslots * 8);
  if (r == hipSuccess) r = hipMemsetAsync(nt->p, 0xFF, nslots * 8, e->stream);
  if (r == hipSuccess) rehash(nt->p, nslots);
  return r;
}

// what every candidate-filling call ends with: the stream's work is done and nothing failed
inline hipError_t finish_stream(JobCtx *e, hipError_t r) {
  const hipError_t rs = hipStreamSynchronize(e->stream);      // (always: kernels that read the candidates may be in flight)
  if (r == hipSuccess) r = rs;
  if (r == hipSuccess) r = hipGetLastError();
  return r;
}

// The table-size ladder of tad_factorize.hip (2^20 -> 2^24 -> 2 V slots, the device says when): attempt(slots, tb, &grow) runs one pass with
// a scratch table of `slots` slots (tb = factorize_temp_bytes) and synchronises once; grow = the pass asked for the next size.
// need_of(tb): the scratch bytes of an attempt, refused above the workspace limit (`slack` more bytes count against the limit without
// appearing in the message).  table: what the caller's message calls the table that cannot fill up.
template <class NeedOf, class Attempt>
int with_factorize_ladder(JobCtx *e, uint64_t V, const char *who, const char *limit_suffix, const char *table, size_t slack, NeedOf need_of, Attempt attempt) {
  for (uint64_t slots = factorize_first_slots(V);;) {
    const size_t tb = factorize_temp_bytes(V, slots);
    const size_t need = need_of(tb);
    if (need + slack > e->ws_limit) return over_limit(e, who, need, limit_suffix);
    bool grow = false;
    const int rc = attempt(slots, tb, &grow);
    if (rc != TAD_OK || !grow) return rc;
    const uint64_t next = factorize_next_slots(V, slots);
    if (next == slots) return fail(e, TAD_ERR_HIP, "%s: the full-size %s filled up", who, table);
    slots = next;
  }
}

// ---- a host batch into device scratch ----
inline size_t key_stage_bytes(const tad_key_columns *kc) {      // every column of every side, then the two masks
  return (size_t)kc->n_cols * (kc->cols_b ? 2 : 1) * up256(kc->n_rows * 8) + 2 * up256(kc->n_rows);
}
// A = the batch kc as the kernels read it.  dst != NULL (a host batch): its columns (a, then b, column by column) and masks are copied to
// dst, key_stage_bytes(kc) bytes; dst == NULL: kc's pointers are device pointers and are used as they are.
inline int stage_key_columns(JobCtx *e, const tad_key_columns *kc, unsigned char *dst, TupleBatch *A) {
  const uint64_t n = kc->n_rows;
  const size_t col_bytes = up256(n * 8), mask_bytes = up256(n);
  hipStream_t s = e->stream;
  *A = TupleBatch{};
  A->keep_a = kc->keep_a; A->keep_b = kc->keep_b; A->n = n; A->n_cols = kc->n_cols; A->sides = kc->cols_b ? 2u : 1u;
  for (int c = 0; c < kc->n_cols; ++c) {
    A->a[c] = reinterpret_cast<const long long *>(kc->cols_a[c]);
    if (A->sides == 2) A->b[c] = reinterpret_cast<const long long *>(kc->cols_b[c]);
  }
  if (dst != nullptr) {
    unsigned char *p = dst;
    for (int c = 0; c < kc->n_cols; ++c) {
      HIP_TRY(e, hipMemcpyAsync(p, kc->cols_a[c], n * 8, hipMemcpyHostToDevice, s)); A->a[c] = reinterpret_cast<const long long *>(p); p += col_bytes;
      if (A->sides == 2) { HIP_TRY(e, hipMemcpyAsync(p, kc->cols_b[c], n * 8, hipMemcpyHostToDevice, s)); A->b[c] = reinterpret_cast<const long long *>(p); p += col_bytes; }
    }
    if (A->keep_a) { HIP_TRY(e, hipMemcpyAsync(p, A->keep_a, n, hipMemcpyHostToDevice, s)); A->keep_a = p; }
    p += mask_bytes;
    if (A->keep_b) { HIP_TRY(e, hipMemcpyAsync(p, A->keep_b, n, hipMemcpyHostToDevice, s)); A->keep_b = p; }
  }
  if (A->sides == 1) A->keep_b = nullptr;
  return TAD_OK;
}

// offsets | bytes (+ slack: the last aligned word a kernel loads) | validity
inline size_t string_stage_bytes(const tad_string_column *col, size_t slack) {
  return up256((col->n_rows + 1) * (col->offset_bits == 64 ? 8 : 4)) + up256(col->data_bytes + slack) +
         (col->validity ? up256((col->validity_offset + col->n_rows + 7) / 8) : 0);
}
// B = the column as the kernels read it; dst != NULL (a host column): copied to dst in the layout above, string_stage_bytes(col, slack) bytes
inline int stage_string_column(JobCtx *e, const tad_string_column *col, unsigned char *dst, size_t slack, StrBatch *B) {
  const uint64_t n = col->n_rows;
  const size_t off_bytes = (n + 1) * (col->offset_bits == 64 ? 8 : 4);
  hipStream_t s = e->stream;
  *B = StrBatch{};
  B->off = col->offsets; B->data = col->data; B->valid = col->validity; B->valid_off = col->validity_offset; B->n = n; B->data_bytes = col->data_bytes;
  B->off64 = col->offset_bits == 64;
  if (dst == nullptr) return TAD_OK;
  unsigned char *p = dst;
  HIP_TRY(e, hipMemcpyAsync(p, col->offsets, off_bytes, hipMemcpyHostToDevice, s)); B->off = p; p += up256(off_bytes);
  if (col->data_bytes) HIP_TRY(e, hipMemcpyAsync(p, col->data, col->data_bytes, hipMemcpyHostToDevice, s));
  B->data = p; p += up256(col->data_bytes + slack);
  if (col->validity) { HIP_TRY(e, hipMemcpyAsync(p, col->validity, (col->validity_offset + n + 7) / 8, hipMemcpyHostToDevice, s)); B->valid = p; }
  return TAD_OK;
}

}  // namespace tadh

#endif  // THEIA_TAD_CAPI_DICT_H
