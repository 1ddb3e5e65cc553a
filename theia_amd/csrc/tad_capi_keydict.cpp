// tad_capi_keydict.cpp — the persistent key dictionary of include/tad.h (tad_keydict_*): the host side of tad_keydict.hip.
// Order of every call that changes the dictionary: check, size, allocate, grow (capacity only) — and only then touch the contents.
#include "tad_capi_dict.h"

using namespace tad;
using namespace tadh;

struct tad_keydict {
  int n_cols = 0;
  uint64_t K = 0;                        // keys held
  unsigned long long *table = nullptr;   // slots words: fingerprint << 32 | id, all ones = empty
  uint64_t slots = 0;                    // a power of two, >= 2 K
  unsigned long long *keys = nullptr;    // key_cap records of kd_stride(n_cols) words
  uint64_t key_cap = 0;
  mutable std::mutex mu;                 // calls on one dictionary are serial (lock order: the dictionary, then a job context)
};

namespace {

constexpr uint64_t kKdMinKeys = 32, kKdDefaultSlots = 1ull << 20, kKdDefaultKeys = 1ull << 16;
constexpr uint64_t kKdMaxKeys = 0xFFFFFFFFull - 1;     // ids < 2^32 - 1

// Room for `total` keys: key records and a table at load <= 1/2.  Capacity only — K, the ids and the tuples are what they were, whether
// this succeeds or not; the old arrays stay the dictionary's until the new ones are complete.
int kd_reserve(JobCtx *e, tad_keydict *d, uint64_t total, uint64_t min_slots = 0) {
  hipStream_t s = e->stream;
  const size_t rec = (size_t)kd_stride(d->n_cols) * 8;
  Candidate<unsigned long long> nkeys, ntable;
  hipError_t r = hipSuccess;
  if (total > d->key_cap) {
    uint64_t ncap = d->key_cap * 2 > total ? d->key_cap * 2 : total;
    if (ncap > kKdMaxKeys) ncap = kKdMaxKeys;
    r = nkeys.alloc(e, ncap, ncap * rec);
    if (r == hipSuccess && d->K) r = hipMemcpyAsync(nkeys.p, d->keys, d->K * rec, hipMemcpyDeviceToDevice, s);
  }
  if (r == hipSuccess)
    r = grow_table(e, d->slots, total, min_slots, &ntable, [&](unsigned long long *t, uint64_t nslots) {
      if (d->K) launch_kd_rehash(s, d->keys, d->n_cols, d->K, t, nslots, nullptr, false);
    });
  if (r == hipSuccess && !nkeys.p && !ntable.p) return TAD_OK;      // room enough
  if (r == hipSuccess) r = hipStreamSynchronize(s);
  if (r == hipSuccess) r = hipGetLastError();
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "tad_keydict: no room for %llu keys: %s (dictionary unchanged)",
                (unsigned long long)total, hipGetErrorString(r));
  nkeys.commit_into(d->keys, d->key_cap);
  ntable.commit_into(d->table, d->slots);
  return TAD_OK;
}

// tad_keydict_encode (insert) / tad_keydict_lookup
int kd_run(tad_engine *eng, tad_keydict *d, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *new_first_row, uint64_t new_first_row_cap,
           uint64_t *num_keys_before, uint64_t *num_keys, bool insert) {
  const char *who = insert ? "tad_keydict_encode" : "tad_keydict_lookup";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || !kc || !kc->cols_a || (kc->n_rows && !key_id) || (kc->cols_b && kc->n_rows && !key_id2) || (new_first_row_cap && !new_first_row))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, key columns, key_id / key_id2 / new_first_row buffers)", who);
  if (kc->n_cols != d->n_cols)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %d key columns, the dictionary holds tuples of %d", who, (int)kc->n_cols, d->n_cols);
  const uint64_t n = kc->n_rows;
  const uint32_t sides = kc->cols_b ? 2 : 1;
  const uint64_t V = n * sides;
  if (V >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %llu virtual rows do not fit 32-bit row indices", who, (unsigned long long)V);
  for (int c = 0; c < kc->n_cols; ++c)
    if (!kc->cols_a[c] || (kc->cols_b && !kc->cols_b[c])) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key column %d is NULL", who, c);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (num_keys_before) *num_keys_before = d->K;
  if (num_keys) *num_keys = d->K;
  if (n == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = kc->memory == TAD_MEM_HOST;
  const int nc = kc->n_cols;
  // scratch of the probe: in_key = a host batch's columns and masks, in_key2 = its ids, sp_comp_a = miss flags | miss count, flags, new-key count
  const size_t col_bytes = up256(n * 8), miss_bytes = up256(V);
  const size_t stage_in = host ? key_stage_bytes(kc) : 0, stage_out = host ? sides * col_bytes : 0;
  const size_t need0 = stage_in + stage_out + miss_bytes + 256;
  if (need0 > e->ws_limit) return over_limit(e, who, need0);
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, miss_bytes + 256)) != TAD_OK) return rc;
  if (host && ((rc = ensure(e, e->in_key, stage_in)) != TAD_OK || (rc = ensure(e, e->in_key2, stage_out)) != TAD_OK)) return rc;
  uint8_t *miss = static_cast<uint8_t *>(e->sp_comp_a.p);
  unsigned char *tail = miss + miss_bytes;
  unsigned long long *n_miss_dev = reinterpret_cast<unsigned long long *>(tail);
  uint32_t *kd_flags_dev = reinterpret_cast<uint32_t *>(tail + 8);
  unsigned long long *nk_dev = reinterpret_cast<unsigned long long *>(tail + 16);
  TupleBatch A;
  if ((rc = stage_key_columns(e, kc, host ? static_cast<unsigned char *>(e->in_key.p) : nullptr, &A)) != TAD_OK) return rc;
  uint64_t *d_key = host ? reinterpret_cast<uint64_t *>(e->in_key2.p) : key_id;
  uint64_t *d_key2 = host && sides == 2 ? d_key + col_bytes / 8 : key_id2;
  auto ids_to_host = [&]() -> int {
    HIP_TRY(e, hipMemcpyAsync(key_id, d_key, n * 8, hipMemcpyDeviceToHost, s));
    if (sides == 2) HIP_TRY(e, hipMemcpyAsync(key_id2, d_key2, n * 8, hipMemcpyDeviceToHost, s));
    return TAD_OK;
  };
  // 1. the probe: the dictionary is only read
  HIP_TRY(e, hipMemsetAsync(tail, 0, 32, s));
  launch_kd_probe(s, A, d->table, d->slots, d->keys, d->K, d_key, d_key2, insert ? miss : nullptr, n_miss_dev);
  unsigned long long M = 0;
  if (insert) HIP_TRY(e, hipMemcpyAsync(&M, n_miss_dev, 8, hipMemcpyDeviceToHost, s));
  if (host && !insert && (rc = ids_to_host()) != TAD_OK) return rc;
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (!insert) return TAD_OK;
  if (M == 0) {      // every tuple known
    if (host) {
      if ((rc = ids_to_host()) != TAD_OK) return rc;
      HIP_TRY(e, hipStreamSynchronize(s));
    }
    return TAD_OK;
  }
  // 2. the miss rows factorised among themselves (keep masks = miss flags): local ids in order of first appearance, the first row of each.
  //    sp_val_a = local ids of both sides, sp_first = first rows (at most one new key per miss row), sp_temp = tad_factorize's scratch
  const size_t loc_bytes = sides * col_bytes, fr_bytes = up256((size_t)M * 8);
  unsigned long long m = 0;
  uint64_t *loc_a = nullptr, *loc_b = nullptr, *fr = nullptr;
  rc = with_factorize_ladder(e, V, who, "", "scratch table", 0, [&](size_t tb) { return need0 + loc_bytes + fr_bytes + tb; }, [&](uint64_t slots, size_t tb, bool *grow) -> int {
    int rc;
    if ((rc = ensure(e, e->sp_val_a, loc_bytes)) != TAD_OK || (rc = ensure(e, e->sp_first, fr_bytes)) != TAD_OK || (rc = ensure(e, e->sp_temp, tb)) != TAD_OK) return rc;
    loc_a = static_cast<uint64_t *>(e->sp_val_a.p);
    loc_b = sides == 2 ? loc_a + col_bytes / 8 : nullptr;
    fr = static_cast<uint64_t *>(e->sp_first.p);
    uint32_t *fz_flags_dev = nullptr;
    launch_factorize(s, A.a, miss, sides == 2 ? A.b : nullptr, sides == 2 ? miss + n : nullptr, n, nc, slots, e->sp_temp.p, loc_a, loc_b, fr, M, nk_dev, &fz_flags_dev);
    uint32_t fz_flags = 0;
    HIP_TRY(e, hipMemcpyAsync(&m, nk_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(&fz_flags, fz_flags_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    *grow = fz_flags != 0;      // more new keys than this scratch table takes
    return TAD_OK;
  });
  if (rc != TAD_OK) return rc;
  if (m == 0 || m > M) return fail(e, TAD_ERR_HIP, "%s: %llu new keys from %llu miss rows", who, (unsigned long long)m, (unsigned long long)M);
  if (d->K + m > kKdMaxKeys)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: %llu keys do not fit 32-bit key ids (dictionary unchanged)", who, (unsigned long long)(d->K + m));
  // room for the new keys: the last step that can fail
  if ((rc = kd_reserve(e, d, d->K + m)) != TAD_OK) return rc;
  // 3. + 4. the new keys' records and slots, the miss rows' ids
  launch_kd_append(s, A, fr, m, d->K, d->table, d->slots, d->keys, kd_flags_dev);
  launch_kd_fix(s, miss, loc_a, loc_b, n, sides, d->K, d_key, d_key2);
  const uint64_t listed = m < new_first_row_cap ? m : new_first_row_cap;
  hipError_t r = hipSuccess;
  if (listed) r = hipMemcpyAsync(new_first_row, fr, listed * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s);
  if (r == hipSuccess && host) {
    r = hipMemcpyAsync(key_id, d_key, n * 8, hipMemcpyDeviceToHost, s);
    if (r == hipSuccess && sides == 2) r = hipMemcpyAsync(key_id2, d_key2, n * 8, hipMemcpyDeviceToHost, s);
  }
  uint32_t kd_flags = 0;
  if (r == hipSuccess) r = hipMemcpyAsync(&kd_flags, kd_flags_dev, 4, hipMemcpyDeviceToHost, s);
  r = finish_stream(e, r);      // (always synchronises: the append is in flight)
  if (r != hipSuccess || (kd_flags & KD_FLAG_BAD_ROW))
    return fail(e, TAD_ERR_HIP, "%s: appending %llu keys failed: %s", who, (unsigned long long)m, hipGetErrorString(r));
  d->K += m;
  if (num_keys) *num_keys = d->K;
  if ((kd_flags & KD_FLAG_CLUSTER) && d->slots < (1ull << 34)) {      // long probe sequences: a table of twice the size, if there is room for one
    if (kd_reserve(e, d, d->K, d->slots * 2) != TAD_OK) (void)hipGetLastError();
  }
  return TAD_OK;
}

}  // namespace

extern "C" {

int tad_keydict_create(tad_engine *eng, int32_t n_cols, uint64_t expected_keys, tad_keydict **out) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_create: engine is NULL");
  if (!out || n_cols < 1 || n_cols > kFzMaxCols || expected_keys > kKdMaxKeys)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_create: bad arguments (1..%d key columns, fewer than 2^32 - 1 keys)", kFzMaxCols);
  *out = nullptr;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_keydict_create: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  tad_keydict *d = new (std::nothrow) tad_keydict();
  if (!d) return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  d->n_cols = n_cols;
  const uint64_t slots = expected_keys ? pow2_at_least(2 * expected_keys) : kKdDefaultSlots;
  const uint64_t key_cap = expected_keys ? (expected_keys > kKdMinKeys ? expected_keys : kKdMinKeys) : kKdDefaultKeys;
  Candidate<unsigned long long> table, keys;
  hipError_t r = table.alloc(e, slots, slots * 8);
  if (r == hipSuccess) r = keys.alloc(e, key_cap, key_cap * (size_t)kd_stride(n_cols) * 8);
  if (r == hipSuccess) r = hipMemsetAsync(table.p, 0xFF, slots * 8, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r != hipSuccess) {
    delete d;
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_keydict_create: %s", hipGetErrorString(r));
  }
  table.commit_into(d->table, d->slots);
  keys.commit_into(d->keys, d->key_cap);
  *out = d;
  return TAD_OK;
}

void tad_keydict_destroy(tad_engine *e, tad_keydict *d) {
  if (!d) return;
  { std::lock_guard<std::mutex> lk(d->mu); }   // a call on this dictionary has returned (it synchronises its stream before it does)
  if (e) hipSetDevice(e->device);
  if (d->table) hipFree(d->table);
  if (d->keys) hipFree(d->keys);
  delete d;
}

int tad_keydict_encode(tad_engine *eng, tad_keydict *d, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *new_first_row,
                       uint64_t new_first_row_cap, uint64_t *num_keys_before, uint64_t *num_keys) {
  return kd_run(eng, d, kc, key_id, key_id2, new_first_row, new_first_row_cap, num_keys_before, num_keys, true);
}

int tad_keydict_lookup(tad_engine *eng, const tad_keydict *d, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2) {
  return kd_run(eng, const_cast<tad_keydict *>(d), kc, key_id, key_id2, nullptr, 0, nullptr, nullptr, false);
}

int tad_keydict_num_keys(tad_engine *eng, const tad_keydict *d, uint64_t *num_keys) {
  if (!eng || !d || !num_keys) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_num_keys: bad arguments");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  *num_keys = d->K;
  return TAD_OK;
}

int tad_keydict_bytes(tad_engine *eng, const tad_keydict *d, uint64_t *bytes) {
  if (!eng || !d || !bytes) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_bytes: bad arguments");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  *bytes = d->slots * 8 + d->key_cap * (uint64_t)kd_stride(d->n_cols) * 8;
  return TAD_OK;
}

int tad_keydict_export(tad_engine *eng, const tad_keydict *d, uint64_t first_key, uint64_t n_keys, int64_t *const *cols, uint8_t *side) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_export: engine is NULL");
  if (!d || (n_keys && !cols)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_export: bad arguments");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (first_key > d->K || n_keys > d->K - first_key)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_export: keys %llu .. %llu of %llu", (unsigned long long)first_key, (unsigned long long)(first_key + n_keys),
                (unsigned long long)d->K);
  if (n_keys == 0) return TAD_OK;
  for (int c = 0; c < d->n_cols; ++c)
    if (!cols[c]) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_export: column %d is NULL", c);
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_keydict_export: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  const size_t stride = (size_t)kd_stride(d->n_cols);
  const uint64_t chunk = n_keys < (1ull << 20) ? n_keys : (1ull << 20);      // records cross the link a chunk at a time
  std::vector<unsigned long long> rows;
  try { rows.resize(chunk * stride); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  for (uint64_t k0 = 0; k0 < n_keys; k0 += chunk) {
    const uint64_t cnt = n_keys - k0 < chunk ? n_keys - k0 : chunk;
    HIP_TRY(e, hipMemcpyAsync(rows.data(), d->keys + (first_key + k0) * stride, cnt * stride * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    for (uint64_t i = 0; i < cnt; ++i) {
      const unsigned long long *rec = rows.data() + i * stride;
      if (side) side[k0 + i] = (uint8_t)rec[0];
      for (int c = 0; c < d->n_cols; ++c) cols[c][k0 + i] = (int64_t)rec[c + 1];
    }
  }
  return TAD_OK;
}

int tad_keydict_import(tad_engine *eng, tad_keydict *d, uint64_t n_keys, const int64_t *const *cols, const uint8_t *side) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: engine is NULL");
  if (!d || (n_keys && !cols) || n_keys > kKdMaxKeys) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: bad arguments (fewer than 2^32 - 1 keys)");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (d->K != 0) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: the dictionary holds %llu keys (import fills an empty one)", (unsigned long long)d->K);
  if (n_keys == 0) return TAD_OK;
  for (int c = 0; c < d->n_cols; ++c)
    if (!cols[c]) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: column %d is NULL", c);
  if (side)
    for (uint64_t i = 0; i < n_keys; ++i)
      if (side[i] > 1) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: side[%llu] = %u (0 = a, 1 = b)", (unsigned long long)i, (unsigned)side[i]);
  const size_t stride = (size_t)kd_stride(d->n_cols);
  std::vector<unsigned long long> rows;
  try { rows.assign(n_keys * stride, 0ull); } catch (...) { return fail(eng, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  for (uint64_t i = 0; i < n_keys; ++i) {
    unsigned long long *rec = rows.data() + i * stride;
    rec[0] = side ? side[i] : 0;
    for (int c = 0; c < d->n_cols; ++c) rec[c + 1] = (unsigned long long)cols[c][i];
  }
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_keydict_import: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, 256)) != TAD_OK) return rc;
  uint32_t *flags_dev = static_cast<uint32_t *>(e->sp_comp_a.p);
  // candidates: they become the dictionary's only when no two tuples are the same
  const uint64_t ncap = n_keys > d->key_cap ? n_keys : d->key_cap;
  uint64_t nslots = pow2_at_least(2 * n_keys);
  if (nslots < d->slots) nslots = d->slots;
  Candidate<unsigned long long> nkeys, ntable;
  hipError_t r = nkeys.alloc(e, ncap, ncap * stride * 8);
  if (r == hipSuccess) r = ntable.alloc(e, nslots, nslots * 8);
  if (r == hipSuccess) r = hipMemcpyAsync(nkeys.p, rows.data(), n_keys * stride * 8, hipMemcpyHostToDevice, s);
  if (r == hipSuccess) r = hipMemsetAsync(ntable.p, 0xFF, nslots * 8, s);
  if (r == hipSuccess) r = hipMemsetAsync(flags_dev, 0, 4, s);
  uint32_t flags = 0;
  if (r == hipSuccess) {
    launch_kd_rehash(s, nkeys.p, d->n_cols, n_keys, ntable.p, nslots, flags_dev, true);
    r = hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, s);
  }
  r = finish_stream(e, r);
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "tad_keydict_import: %s (dictionary unchanged)", hipGetErrorString(r));
  if (flags != 0) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_import: two keys hold the same tuple (dictionary unchanged)");
  nkeys.commit_into(d->keys, d->key_cap);
  ntable.commit_into(d->table, d->slots);
  d->K = n_keys;
  return TAD_OK;
}

// tad.h: a key mask from the dictionary's tuples (kernel: k_kd_select).  The dictionary is only read.
int tad_keydict_select(tad_engine *eng, const tad_keydict *d, int32_t n_terms, const int32_t *term_col, const uint8_t *const *masks, const uint64_t *mask_len,
                       int32_t side, uint8_t *key_keep, uint64_t key_keep_len, tad_mem memory, uint64_t *n_selected) {
  const char *who = "tad_keydict_select";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || n_terms < 0 || n_terms > kKdMaxTerms || (n_terms && (!term_col || !masks || !mask_len)) || side < -1 || side > 1 || (key_keep_len && !key_keep) ||
      (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, 0..%d terms, side -1 / 0 / 1, key_keep buffer in host or device memory)", who,
                kKdMaxTerms);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  for (int t = 0; t < n_terms; ++t) {
    if (term_col[t] < 0 || term_col[t] >= d->n_cols)
      return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: term %d names column %d, the dictionary holds tuples of %d", who, t, (int)term_col[t], d->n_cols);
    if (mask_len[t] && !masks[t]) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the mask of term %d is NULL", who, t);
  }
  if (key_keep_len != K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep has %llu entries, the dictionary holds %llu keys", who, (unsigned long long)key_keep_len,
                (unsigned long long)K);
  if (n_selected) *n_selected = 0;
  if (K == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  // scratch: sp_comp_a = the selected count | flags; a host call's masks in in_key and its key_keep in in_key2
  size_t stage_in = 0;
  if (host)
    for (int t = 0; t < n_terms; ++t) stage_in += up256(mask_len[t]);
  const size_t need = 256 + (host ? stage_in + up256(K) : 0);
  if (need > e->ws_limit) return over_limit(e, who, need);
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, 256)) != TAD_OK) return rc;
  if (host && ((stage_in && (rc = ensure(e, e->in_key, stage_in)) != TAD_OK) || (rc = ensure(e, e->in_key2, up256(K))) != TAD_OK)) return rc;
  unsigned long long *n_sel_dev = static_cast<unsigned long long *>(e->sp_comp_a.p);
  uint32_t *flags_dev = reinterpret_cast<uint32_t *>(n_sel_dev + 1);
  KdSelect q{};
  q.n_terms = n_terms;
  q.side = side;
  unsigned char *p = host && stage_in ? static_cast<unsigned char *>(e->in_key.p) : nullptr;
  for (int t = 0; t < n_terms; ++t) {
    q.col[t] = term_col[t];
    q.mask_len[t] = mask_len[t];
    q.mask[t] = masks[t];
    if (host && mask_len[t]) {
      HIP_TRY(e, hipMemcpyAsync(p, masks[t], mask_len[t], hipMemcpyHostToDevice, s));
      q.mask[t] = p;
      p += up256(mask_len[t]);
    }
  }
  uint8_t *d_keep = host ? static_cast<uint8_t *>(e->in_key2.p) : key_keep;
  HIP_TRY(e, hipMemsetAsync(n_sel_dev, 0, 16, s));
  launch_kd_select(s, d->keys, d->n_cols, K, q, d_keep, n_sel_dev, flags_dev);
  unsigned long long n_sel = 0;
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&n_sel, n_sel_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, s));
  if (host) HIP_TRY(e, hipMemcpyAsync(key_keep, d_keep, K, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (flags & KD_FLAG_BAD_CODE) return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: a key's value lies outside the mask of its term (key_keep unspecified)", who);
  if (n_selected) *n_selected = n_sel;
  return TAD_OK;
}

// tad.h: ids -> tuples (kernel: k_kd_gather).  The dictionary is only read.
int tad_keydict_gather(tad_engine *eng, const tad_keydict *d, const uint64_t *key_id, uint64_t n, tad_mem memory, int64_t *const *cols, uint8_t *side) {
  const char *who = "tad_keydict_gather";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (n && (!key_id || !cols)) || (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, key_id, the array of column pointers, host or device memory)", who);
  if (n >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %llu ids do not fit 32-bit row indices", who, (unsigned long long)n);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (n == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  unsigned col_mask = 0;
  for (int c = 0; c < d->n_cols; ++c)
    if (cols[c]) col_mask |= 1u << c;
  // scratch: in_key = the flag word; a host call's ids, asked columns and sides behind it (kd_gather_layout)
  Carve measure(nullptr);
  kd_gather_layout(measure, n, d->n_cols, col_mask, side != nullptr, host);
  if (measure.bytes() > e->ws_limit) return over_limit(e, who, measure.bytes());
  int rc;
  if ((rc = ensure(e, e->in_key, measure.bytes())) != TAD_OK) return rc;
  Carve place(e->in_key.p);
  const KdGatherWs w = kd_gather_layout(place, n, d->n_cols, col_mask, side != nullptr, host);
  KdGatherOut o{};
  for (int c = 0; c < d->n_cols; ++c) o.col[c] = host ? w.col[c] : reinterpret_cast<long long *>(cols[c]);
  o.side = host ? w.side : side;
  HIP_TRY(e, hipMemsetAsync(w.flags, 0, 4, s));
  if (host) HIP_TRY(e, hipMemcpyAsync(w.ids, key_id, n * 8, hipMemcpyHostToDevice, s));
  launch_kd_gather(s, d->keys, d->n_cols, d->K, host ? reinterpret_cast<const uint64_t *>(w.ids) : key_id, n, o, w.flags);
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&flags, w.flags, 4, hipMemcpyDeviceToHost, s));
  if (host) {
    for (int c = 0; c < d->n_cols; ++c)
      if (cols[c]) HIP_TRY(e, hipMemcpyAsync(cols[c], w.col[c], n * 8, hipMemcpyDeviceToHost, s));
    if (side) HIP_TRY(e, hipMemcpyAsync(side, w.side, n, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (flags & KD_FLAG_BAD_ID)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: an id is not below the %llu keys held (TAD_KEY_SKIP is no key; the outputs are unspecified)", who,
                (unsigned long long)d->K);
  return TAD_OK;
}

// tad.h: the renumbering of tad_state_compact applied to the dictionary (kernels in tad_compact.hip).  The check runs first and alone;
// then fresh records and a fresh table are filled and swapped in.
int tad_keydict_compact(tad_engine *eng, tad_keydict *d, const uint64_t *remap, uint64_t remap_len, tad_mem remap_memory, uint64_t *num_keys) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_compact: engine is NULL");
  if (!d || (remap_len && !remap) || (remap_memory != TAD_MEM_HOST && remap_memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_compact: bad arguments (dictionary, remap in host or device memory); dictionary unchanged");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  if (remap_len != K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_compact: remap has %llu entries, the dictionary holds %llu keys (dictionary unchanged)",
                (unsigned long long)remap_len, (unsigned long long)K);
  if (num_keys) *num_keys = K;
  if (K == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_keydict_compact: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = remap_memory == TAD_MEM_HOST;
  // scratch: in_key = a host remap; sp_comp_a = live flags | error word; sp_val_a = survivors below, K + 1
  const size_t live_bytes = up256(K * 4), below_bytes = up256((K + 1) * 8), scan_bytes = scan_scratch_elems(K) * sizeof(unsigned long long);
  const size_t need = (host ? up256(K * 8) : 0) + live_bytes + 256 + below_bytes + scan_bytes;
  if (need > e->ws_limit) return over_limit(e, "tad_keydict_compact", need, " (dictionary unchanged)");
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, live_bytes + 256)) != TAD_OK || (rc = ensure(e, e->sp_val_a, below_bytes)) != TAD_OK ||
      (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK || (host && (rc = ensure(e, e->in_key, up256(K * 8))) != TAD_OK))
    return rc;
  uint32_t *live = static_cast<uint32_t *>(e->sp_comp_a.p);
  uint32_t *err_dev = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(e->sp_comp_a.p) + live_bytes);
  unsigned long long *below = static_cast<unsigned long long *>(e->sp_val_a.p);
  const unsigned long long *d_remap = reinterpret_cast<const unsigned long long *>(remap);
  if (host) {
    HIP_TRY(e, hipMemcpyAsync(e->in_key.p, remap, K * 8, hipMemcpyHostToDevice, s));
    d_remap = static_cast<const unsigned long long *>(e->in_key.p);
  }
  // 1. the check: the kept entries are 0, 1, ..., m - 1 in order.  The dictionary is only read
  HIP_TRY(e, hipMemsetAsync(err_dev, 0, 4, s));
  launch_kd_live(s, d_remap, K, live);
  launch_scan(s, live, below, K, static_cast<unsigned long long *>(e->scan_scratch.p));
  launch_kd_compact(s, d_remap, below, K, d->keys, d->n_cols, nullptr, err_dev);
  unsigned long long m = 0;
  uint32_t err = 0;
  HIP_TRY(e, hipMemcpyAsync(&m, below + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&err, err_dev, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (err != 0 || m > K)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_keydict_compact: the entries of remap that are not TAD_KEY_SKIP must be 0, 1, ..., m - 1 in order "
                                             "(what tad_state_compact writes); dictionary unchanged");
  if (m == K) return TAD_OK;      // the identity: nothing leaves
  // 2. fresh records and a fresh table, at the size tad_keydict_create(expected_keys = 2 m) picks and never above the current one
  const size_t rec = (size_t)kd_stride(d->n_cols) * 8;
  uint64_t ncap = 2 * m > kKdMinKeys ? 2 * m : kKdMinKeys, nslots = pow2_at_least(4 * m);
  if (ncap > d->key_cap) ncap = d->key_cap;
  if (nslots > d->slots) nslots = d->slots;
  Candidate<unsigned long long> nkeys, ntable;
  hipError_t r = nkeys.alloc(e, ncap, ncap * rec);
  if (r == hipSuccess) r = ntable.alloc(e, nslots, nslots * 8);
  if (r == hipSuccess) r = hipMemsetAsync(ntable.p, 0xFF, nslots * 8, s);
  if (r == hipSuccess) {
    launch_kd_compact(s, d_remap, below, K, d->keys, d->n_cols, nkeys.p, err_dev);
    if (m) launch_kd_rehash(s, nkeys.p, d->n_cols, m, ntable.p, nslots, nullptr, false);
    r = hipStreamSynchronize(s);
  }
  if (r == hipSuccess) r = hipGetLastError();
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "tad_keydict_compact: %s (dictionary unchanged)", hipGetErrorString(r));
  nkeys.commit_into(d->keys, d->key_cap);
  ntable.commit_into(d->table, d->slots);
  d->K = m;
  if (num_keys) *num_keys = m;
  return TAD_OK;
}

// tad.h: which codes of a column do the keys still hold (kernels: k_kd_mark, k_kd_count_used).  The dictionary is only read.
int tad_keydict_mark_codes(tad_engine *eng, const tad_keydict *d, int32_t col, int32_t accumulate, uint8_t *used, uint64_t used_len, tad_mem memory,
                           uint64_t *n_used) {
  const char *who = "tad_keydict_mark_codes";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (used_len && !used) || (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, used buffer in host or device memory)", who);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (col < 0 || col >= d->n_cols)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: column %d, the dictionary holds tuples of %d", who, (int)col, d->n_cols);
  const uint64_t K = d->K;
  if (used_len == 0 && K == 0) {
    if (n_used) *n_used = 0;
    return TAD_OK;
  }
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  // scratch: in_key = the count | the flag word | a host call's used bytes (kd_mark_layout)
  Carve measure(nullptr);
  kd_mark_layout(measure, used_len, host);
  if (measure.bytes() > e->ws_limit) return over_limit(e, who, measure.bytes());
  int rc;
  if ((rc = ensure(e, e->in_key, measure.bytes())) != TAD_OK) return rc;
  Carve place(e->in_key.p);
  const KdMarkWs w = kd_mark_layout(place, used_len, host);
  uint8_t *d_used = host ? w.used : used;
  HIP_TRY(e, hipMemsetAsync(w.n_used, 0, 16, s));
  if (used_len) {
    if (!accumulate) HIP_TRY(e, hipMemsetAsync(d_used, 0, used_len, s));
    else if (host) HIP_TRY(e, hipMemcpyAsync(d_used, used, used_len, hipMemcpyHostToDevice, s));
  }
  launch_kd_mark(s, d->keys, d->n_cols, K, col, d_used, used_len, w.flags);
  launch_kd_count_used(s, d_used, used_len, w.n_used);
  unsigned long long count = 0;
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&count, w.n_used, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&flags, w.flags, 4, hipMemcpyDeviceToHost, s));
  if (host && used_len) HIP_TRY(e, hipMemcpyAsync(used, d_used, used_len, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (flags & KD_FLAG_BAD_CODE)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: a key's value in column %d lies outside the %llu entries of used (used unspecified)", who, (int)col,
                (unsigned long long)used_len);
  if (n_used) *n_used = count;
  return TAD_OK;
}

// tad.h: the keys' columns passed through code remaps (kernels: k_kd_recode, k_kd_rehash).  The check runs first and alone; then fresh
// records and a fresh table are filled — two keys with one recoded tuple are found there — and swapped in.
int tad_keydict_recode(tad_engine *eng, tad_keydict *d, int32_t n_terms, const int32_t *term_col, const int64_t *const *remaps, const uint64_t *remap_len,
                       tad_mem memory, uint64_t *num_keys) {
  const char *who = "tad_keydict_recode";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || n_terms < 0 || n_terms > kKdMaxTerms || (n_terms && (!term_col || !remaps || !remap_len)) || (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, 0..%d terms, remaps in host or device memory); dictionary unchanged", who, kKdMaxTerms);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  for (int t = 0; t < n_terms; ++t) {
    if (term_col[t] < 0 || term_col[t] >= d->n_cols)
      return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: term %d names column %d, the dictionary holds tuples of %d (dictionary unchanged)", who, t, (int)term_col[t],
                  d->n_cols);
    for (int u = 0; u < t; ++u)
      if (term_col[u] == term_col[t])
        return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: terms %d and %d both name column %d (dictionary unchanged)", who, u, t, (int)term_col[t]);
    if (remap_len[t] && !remaps[t]) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the remap of term %d is NULL (dictionary unchanged)", who, t);
  }
  auto done = [&]() {      // the output is written by a call that succeeds, and by no other
    if (num_keys) *num_keys = K;
    return TAD_OK;
  };
  if (K == 0 || n_terms == 0) return done();
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  // scratch: in_key = the flag word | a host call's remaps (kd_recode_layout)
  Carve measure(nullptr);
  kd_recode_layout(measure, n_terms, remap_len, host);
  if (measure.bytes() > e->ws_limit) return over_limit(e, who, measure.bytes(), " (dictionary unchanged)");
  int rc;
  if ((rc = ensure(e, e->in_key, measure.bytes())) != TAD_OK) return rc;
  Carve place(e->in_key.p);
  const KdRecodeWs w = kd_recode_layout(place, n_terms, remap_len, host);
  KdRecode q{};
  q.n_terms = n_terms;
  for (int t = 0; t < n_terms; ++t) {
    q.col[t] = term_col[t];
    q.len[t] = remap_len[t];
    q.remap[t] = reinterpret_cast<const long long *>(remaps[t]);
    if (host) {
      if (remap_len[t]) HIP_TRY(e, hipMemcpyAsync(w.remap[t], remaps[t], remap_len[t] * 8, hipMemcpyHostToDevice, s));
      q.remap[t] = w.remap[t];
    }
  }
  // 1. the check: every value has a new code.  The dictionary is only read
  HIP_TRY(e, hipMemsetAsync(w.flags, 0, 4, s));
  launch_kd_recode(s, d->keys, d->n_cols, K, q, nullptr, w.flags);
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&flags, w.flags, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (flags & KD_FLAG_BAD_CODE)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: a key's value lies outside the remap of its column or maps to TAD_CODE_NONE — the key still uses a retired "
                                             "value (dictionary unchanged)", who);
  if (!(flags & KD_FLAG_CHANGED)) return done();      // the identity on every value held: nothing moves
  // 2. fresh records and a fresh table of the current sizes
  const size_t rec = (size_t)kd_stride(d->n_cols) * 8;
  Candidate<unsigned long long> nkeys, ntable;
  hipError_t r = nkeys.alloc(e, d->key_cap, d->key_cap * rec);
  if (r == hipSuccess) r = ntable.alloc(e, d->slots, d->slots * 8);
  if (r == hipSuccess) r = hipMemsetAsync(ntable.p, 0xFF, d->slots * 8, s);
  if (r == hipSuccess) r = hipMemsetAsync(w.flags, 0, 4, s);
  if (r == hipSuccess) {
    launch_kd_recode(s, d->keys, d->n_cols, K, q, nkeys.p, w.flags);
    launch_kd_rehash(s, nkeys.p, d->n_cols, K, ntable.p, d->slots, w.flags, true);
    r = hipMemcpyAsync(&flags, w.flags, 4, hipMemcpyDeviceToHost, s);
  }
  r = finish_stream(e, r);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "%s: %s (dictionary unchanged)", who, hipGetErrorString(r));
  }
  if (flags & KD_FLAG_DUPLICATE) return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: two keys hold the same tuple after recoding (dictionary unchanged)", who);
  nkeys.commit_into(d->keys, d->key_cap);
  ntable.commit_into(d->table, d->slots);
  return done();
}

}  // extern "C"
