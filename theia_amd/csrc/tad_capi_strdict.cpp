// tad_capi_strdict.cpp — the persistent string dictionary of include/tad.h (tad_strdict_*): the host side of tad_strdict.hip.
// Order of every call that changes the dictionary: check, probe (the offsets are validated there), size, allocate, grow (capacity only) —
// and only then touch the contents.
#include "tad_capi_dict.h"

using namespace tad;
using namespace tadh;

struct tad_strdict {
  uint64_t K = 0;                        // values held
  unsigned long long *table = nullptr;   // slots words: fingerprint << 32 | code, all ones = empty
  uint64_t slots = 0;                    // a power of two, >= 2 K
  void *recs = nullptr;                  // rec_cap records of 16 bytes: arena offset | hash's low half << 32 | length
  uint64_t rec_cap = 0;
  uint8_t *arena = nullptr;              // the strings, each 16-byte aligned and zero-padded to a multiple of 16
  uint64_t arena_cap = 0, arena_used = 0;   // multiples of 16
  mutable std::mutex mu;                 // calls on one dictionary are serial (lock order: the dictionary, then a job context)
};

namespace {

constexpr uint64_t kSdMinValues = 32, kSdDefaultSlots = 1ull << 20, kSdDefaultValues = 1ull << 16, kSdDefaultArena = 4ull << 20;
constexpr uint64_t kSdMaxValues = 0xFFFFFFFFull - 1;     // codes < 2^32 - 1
constexpr uint64_t kNoCount = ~0ull;

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// Room for `total` values and `bytes` arena bytes: records, arena and a table at load <= 1/2.  Capacity only — K, the codes and the strings
// are what they were, whether this succeeds or not; the old arrays stay the dictionary's until the new ones are complete.
int sd_reserve(JobCtx *e, tad_strdict *d, uint64_t total, uint64_t bytes, uint64_t min_slots = 0) {
  hipStream_t s = e->stream;
  Candidate<void> nrecs;
  Candidate<uint8_t> narena;
  Candidate<unsigned long long> ntable;
  hipError_t r = hipSuccess;
  if (total > d->rec_cap) {
    uint64_t ncap = d->rec_cap * 2 > total ? d->rec_cap * 2 : total;
    if (ncap > kSdMaxValues) ncap = kSdMaxValues;
    r = nrecs.alloc(e, ncap, ncap * 16);
  }
  if (r == hipSuccess && bytes > d->arena_cap) {
    const uint64_t ncap = up16(d->arena_cap * 2 > bytes ? d->arena_cap * 2 : bytes);
    r = narena.alloc(e, ncap, ncap);
  }
  if (r == hipSuccess && nrecs.p && d->K) r = hipMemcpyAsync(nrecs.p, d->recs, d->K * 16, hipMemcpyDeviceToDevice, s);
  if (r == hipSuccess && narena.p && d->arena_used) r = hipMemcpyAsync(narena.p, d->arena, d->arena_used, hipMemcpyDeviceToDevice, s);
  if (r == hipSuccess)
    r = grow_table(e, d->slots, total, min_slots, &ntable, [&](unsigned long long *t, uint64_t nslots) {
      if (d->K) launch_sd_rehash(s, d->table, d->slots, d->recs, d->K, t, nslots);
    });
  if (r == hipSuccess && !nrecs.p && !narena.p && !ntable.p) return TAD_OK;      // room enough
  if (r == hipSuccess) r = hipStreamSynchronize(s);
  if (r == hipSuccess) r = hipGetLastError();
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "tad_strdict: no room for %llu values, %llu bytes: %s (dictionary unchanged)",
                (unsigned long long)total, (unsigned long long)bytes, hipGetErrorString(r));
  nrecs.commit_into(d->recs, d->rec_cap);
  narena.commit_into(d->arena, d->arena_cap);
  ntable.commit_into(d->table, d->slots);
  return TAD_OK;
}

// tad_strdict_encode (insert) / tad_strdict_lookup / tad_strdict_import (insert, must_be_new = the rows: every row a new value).  The caller
// holds the dictionary's lock.
int sd_run(tad_engine *eng, tad_strdict *d, const tad_string_column *col, int64_t *codes, uint64_t *new_first_row, uint64_t new_first_row_cap, uint64_t *num_before,
           uint64_t *num_values, bool insert, uint64_t must_be_new, const char *who) {
  const uint64_t n = col->n_rows;
  if (num_before) *num_before = d->K;
  if (num_values) *num_values = d->K;
  if (n == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = col->memory == TAD_MEM_HOST;
  // scratch of the probe: in_key = a host batch's offsets | bytes (+ 16 of slack: the last aligned word) | validity, in_key2 = its codes,
  // sp_comp_a = miss flags | miss count, probe flags, new-value count, append flags
  const size_t stage_in = host ? string_stage_bytes(col, 16) : 0, stage_out = host ? up256(n * 8) : 0, miss_bytes = up256(n);
  const size_t need0 = stage_in + stage_out + miss_bytes + 256;
  if (need0 > e->ws_limit) return over_limit(e, who, need0);
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, miss_bytes + 256)) != TAD_OK) return rc;
  if (host && ((rc = ensure(e, e->in_key, stage_in)) != TAD_OK || (rc = ensure(e, e->in_key2, stage_out)) != TAD_OK)) return rc;
  uint8_t *miss = static_cast<uint8_t *>(e->sp_comp_a.p);
  unsigned char *tail = miss + miss_bytes;
  unsigned long long *n_miss_dev = reinterpret_cast<unsigned long long *>(tail);
  uint32_t *probe_flags_dev = reinterpret_cast<uint32_t *>(tail + 8);
  unsigned long long *nv_dev = reinterpret_cast<unsigned long long *>(tail + 16);
  uint32_t *append_flags_dev = reinterpret_cast<uint32_t *>(tail + 24);
  StrBatch B;
  if ((rc = stage_string_column(e, col, host ? static_cast<unsigned char *>(e->in_key.p) : nullptr, 16, &B)) != TAD_OK) return rc;
  long long *d_codes = reinterpret_cast<long long *>(host ? e->in_key2.p : codes);
  // 1. the probe: the dictionary is only read; every row's offsets are validated
  HIP_TRY(e, hipMemsetAsync(tail, 0, 32, s));
  launch_sd_probe(s, B, d->table, d->slots, d->recs, d->arena, d->K, d_codes, insert ? miss : nullptr, n_miss_dev, probe_flags_dev);
  unsigned long long M = 0;
  uint32_t probe_flags = 0;
  if (insert) HIP_TRY(e, hipMemcpyAsync(&M, n_miss_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&probe_flags, probe_flags_dev, 4, hipMemcpyDeviceToHost, s));
  if (host && !insert) HIP_TRY(e, hipMemcpyAsync(codes, d_codes, n * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (probe_flags & SD_FLAG_BAD_OFFSETS) return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: offsets decrease or point beyond data_bytes (dictionary unchanged)", who);
  if (!insert) return TAD_OK;
  if (must_be_new != kNoCount && M != must_be_new)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: %llu of %llu strings are already held (dictionary unchanged)", who, (unsigned long long)(must_be_new - M),
                (unsigned long long)must_be_new);
  if (M == 0) {      // every string known
    if (host) {
      HIP_TRY(e, hipMemcpyAsync(codes, d_codes, n * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(e, hipStreamSynchronize(s));
    }
    return TAD_OK;
  }
  // 2. the miss rows de-duplicated among themselves (keep mask = miss flags): local ids in order of first appearance into the miss rows of the
  //    output, the first row of each.  3. the new values' padded lengths scanned into arena offsets (16-byte units).
  //    sp_temp = tad_encode_strings' scratch, sp_first = first rows (at most one new value per miss row), sp_val_a = units | offsets
  const size_t fr_bytes = up256((size_t)M * 8), cnt_bytes = up256((size_t)M * 4), offs_bytes = up256(((size_t)M + 1) * 8);
  const size_t scan_bytes = scan_scratch_elems(M) * sizeof(unsigned long long);
  unsigned long long m = 0, units = 0;
  uint64_t *fr = nullptr;
  unsigned long long *off16 = nullptr;
  rc = with_factorize_ladder(e, n, who, " (dictionary unchanged)", "scratch table", 0, [&](size_t tb) { return need0 + tb + fr_bytes + cnt_bytes + offs_bytes + scan_bytes; },
                             [&](uint64_t slots, size_t tb, bool *grow) -> int {
    int rc;
    if ((rc = ensure(e, e->sp_temp, tb)) != TAD_OK || (rc = ensure(e, e->sp_first, fr_bytes)) != TAD_OK || (rc = ensure(e, e->sp_val_a, cnt_bytes + offs_bytes)) != TAD_OK ||
        (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK)
      return rc;
    fr = static_cast<uint64_t *>(e->sp_first.p);
    uint32_t *cnt = static_cast<uint32_t *>(e->sp_val_a.p);
    off16 = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->sp_val_a.p) + cnt_bytes);
    uint32_t *se_flags_dev = nullptr;
    launch_encode_strings(s, B.off, B.off64, B.data, B.data_bytes, B.valid, B.valid_off, n, slots, e->sp_temp.p, d_codes, fr, M, nv_dev, &se_flags_dev, miss);
    launch_sd_lens(s, B, fr, nv_dev, M, se_flags_dev, cnt);
    launch_scan(s, cnt, off16, M, static_cast<unsigned long long *>(e->scan_scratch.p));
    uint32_t se_flags = 0;
    HIP_TRY(e, hipMemcpyAsync(&m, nv_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(&units, off16 + M, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(&se_flags, se_flags_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    if (se_flags & 2u) return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: offsets decrease or point beyond data_bytes (dictionary unchanged)", who);
    *grow = se_flags != 0;      // more new values than this scratch table takes
    return TAD_OK;
  });
  if (rc != TAD_OK) return rc;
  if (m == 0 || m > M) return fail(e, TAD_ERR_HIP, "%s: %llu new values from %llu miss rows", who, (unsigned long long)m, (unsigned long long)M);
  if (must_be_new != kNoCount && m != must_be_new)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: two strings are equal (%llu distinct of %llu; dictionary unchanged)", who, (unsigned long long)m,
                (unsigned long long)must_be_new);
  if (d->K + m > kSdMaxValues)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: %llu values do not fit 32-bit codes (dictionary unchanged)", who, (unsigned long long)(d->K + m));
  const uint64_t new_bytes = units * 16ull;
  // room for the new values: the last step that can fail
  if ((rc = sd_reserve(e, d, d->K + m, d->arena_used + new_bytes)) != TAD_OK) return rc;
  // 4. + 5. the new values' bytes, records and slots, the miss rows' codes
  launch_sd_append(s, B, fr, off16, m, d->K, d->arena_used, d->table, d->slots, d->recs, d->arena, append_flags_dev);
  launch_sd_fix(s, miss, n, d->K, d_codes);
  const uint64_t listed = m < new_first_row_cap ? m : new_first_row_cap;
  hipError_t r = hipSuccess;
  if (listed) r = hipMemcpyAsync(new_first_row, fr, listed * 8, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s);
  if (r == hipSuccess && host) r = hipMemcpyAsync(codes, d_codes, n * 8, hipMemcpyDeviceToHost, s);
  uint32_t append_flags = 0;
  if (r == hipSuccess) r = hipMemcpyAsync(&append_flags, append_flags_dev, 4, hipMemcpyDeviceToHost, s);
  r = finish_stream(e, r);      // (always synchronises: the append is in flight)
  if (r != hipSuccess || (append_flags & SD_FLAG_BAD_ROW))
    return fail(e, TAD_ERR_HIP, "%s: appending %llu values failed: %s", who, (unsigned long long)m, hipGetErrorString(r));
  d->K += m;
  d->arena_used += new_bytes;
  if (num_values) *num_values = d->K;
  if ((append_flags & SD_FLAG_CLUSTER) && d->slots < (1ull << 34)) {      // long probe sequences: a table of twice the size, if there is room for one
    if (sd_reserve(e, d, d->K, d->arena_used, d->slots * 2) != TAD_OK) (void)hipGetLastError();
  }
  return TAD_OK;
}

int sd_check_column(tad_engine *eng, const tad_strdict *d, const tad_string_column *col, const int64_t *codes, const uint64_t *new_first_row, uint64_t new_first_row_cap,
                    const char *who) {
  if (!d || !col || (col->offset_bits != 32 && col->offset_bits != 64) || (col->n_rows && (!col->offsets || !codes)) || (new_first_row_cap && !new_first_row) ||
      (col->data_bytes && !col->data) || (col->memory != TAD_MEM_HOST && col->memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, offsets of 32 or 64 bits, data, codes / new_first_row buffers in host or device memory)", who);
  if (col->n_rows >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %llu rows do not fit 32-bit row indices", who, (unsigned long long)col->n_rows);
  return TAD_OK;
}

}  // namespace

extern "C" {

int tad_strdict_create(tad_engine *eng, uint64_t expected_values, uint64_t expected_bytes, tad_strdict **out) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_create: engine is NULL");
  if (!out || expected_values > kSdMaxValues) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_create: bad arguments (fewer than 2^32 - 1 values)");
  *out = nullptr;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_strdict_create: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  tad_strdict *d = new (std::nothrow) tad_strdict();
  if (!d) return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  const uint64_t slots = expected_values ? pow2_at_least(2 * expected_values) : kSdDefaultSlots;
  const uint64_t rec_cap = expected_values ? (expected_values > kSdMinValues ? expected_values : kSdMinValues) : kSdDefaultValues;
  const uint64_t arena_cap = expected_bytes ? up16(expected_bytes) : kSdDefaultArena;
  Candidate<unsigned long long> table;
  Candidate<void> recs;
  Candidate<uint8_t> arena;
  hipError_t r = table.alloc(e, slots, slots * 8);
  if (r == hipSuccess) r = recs.alloc(e, rec_cap, rec_cap * 16);
  if (r == hipSuccess) r = arena.alloc(e, arena_cap, arena_cap);
  if (r == hipSuccess) r = hipMemsetAsync(table.p, 0xFF, slots * 8, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r != hipSuccess) {
    delete d;
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_strdict_create: %s", hipGetErrorString(r));
  }
  table.commit_into(d->table, d->slots);
  recs.commit_into(d->recs, d->rec_cap);
  arena.commit_into(d->arena, d->arena_cap);
  *out = d;
  return TAD_OK;
}

void tad_strdict_destroy(tad_engine *e, tad_strdict *d) {
  if (!d) return;
  { std::lock_guard<std::mutex> lk(d->mu); }   // a call on this dictionary has returned (it synchronises its stream before it does)
  if (e) hipSetDevice(e->device);
  if (d->table) hipFree(d->table);
  if (d->recs) hipFree(d->recs);
  if (d->arena) hipFree(d->arena);
  delete d;
}

int tad_strdict_encode(tad_engine *eng, tad_strdict *d, const tad_string_column *col, int64_t *codes, uint64_t *new_first_row, uint64_t new_first_row_cap,
                       uint64_t *num_before, uint64_t *num_values) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_encode: engine is NULL");
  int rc;
  if ((rc = sd_check_column(eng, d, col, codes, new_first_row, new_first_row_cap, "tad_strdict_encode")) != TAD_OK) return rc;
  std::lock_guard<std::mutex> dict_lk(d->mu);
  return sd_run(eng, d, col, codes, new_first_row, new_first_row_cap, num_before, num_values, true, kNoCount, "tad_strdict_encode");
}

int tad_strdict_lookup(tad_engine *eng, const tad_strdict *d, const tad_string_column *col, int64_t *codes) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_lookup: engine is NULL");
  int rc;
  if ((rc = sd_check_column(eng, d, col, codes, nullptr, 0, "tad_strdict_lookup")) != TAD_OK) return rc;
  std::lock_guard<std::mutex> dict_lk(d->mu);
  return sd_run(eng, const_cast<tad_strdict *>(d), col, codes, nullptr, 0, nullptr, nullptr, false, kNoCount, "tad_strdict_lookup");
}

int tad_strdict_num_values(tad_engine *eng, const tad_strdict *d, uint64_t *num_values) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_num_values: engine is NULL");
  if (!d || !num_values) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_num_values: bad arguments");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  *num_values = d->K;
  return TAD_OK;
}

int tad_strdict_bytes(tad_engine *eng, const tad_strdict *d, uint64_t *bytes) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_bytes: engine is NULL");
  if (!d || !bytes) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_strdict_bytes: bad arguments");
  std::lock_guard<std::mutex> dict_lk(d->mu);
  *bytes = d->slots * 8 + d->rec_cap * 16 + d->arena_cap;
  return TAD_OK;
}

int tad_strdict_export(tad_engine *eng, const tad_strdict *d, uint64_t first_code, uint64_t n_values, int64_t *offsets, uint8_t *data, uint64_t data_cap,
                       uint64_t *data_bytes) {
  const char *who = "tad_strdict_export";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (!offsets && data) || (data_cap && !data)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, offsets with data)", who);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (first_code > d->K || n_values > d->K - first_code)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: values %llu .. %llu of %llu", who, (unsigned long long)first_code, (unsigned long long)(first_code + n_values),
                (unsigned long long)d->K);
  const bool query = !offsets && !data;
  if (n_values == 0) {
    if (data_bytes) *data_bytes = 0;
    if (offsets) offsets[0] = 0;
    return TAD_OK;
  }
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  // scratch: sp_val_a = lengths | offsets, sp_temp = the packed bytes
  const size_t cnt_bytes = up256((size_t)n_values * 4), offs_bytes = up256(((size_t)n_values + 1) * 8);
  const size_t scan_bytes = scan_scratch_elems(n_values) * sizeof(unsigned long long);
  if (cnt_bytes + offs_bytes + scan_bytes > e->ws_limit) return over_limit(e, who, cnt_bytes + offs_bytes + scan_bytes);
  int rc;
  if ((rc = ensure(e, e->sp_val_a, cnt_bytes + offs_bytes)) != TAD_OK || (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK) return rc;
  uint32_t *cnt = static_cast<uint32_t *>(e->sp_val_a.p);
  unsigned long long *off = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->sp_val_a.p) + cnt_bytes);
  launch_sd_export_lens(s, d->recs, first_code, n_values, cnt);
  launch_scan(s, cnt, off, n_values, static_cast<unsigned long long *>(e->scan_scratch.p));
  unsigned long long total = 0;
  HIP_TRY(e, hipMemcpyAsync(&total, off + n_values, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (data_bytes) *data_bytes = total;
  if (query) return TAD_OK;
  if (total > data_cap)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: the values hold %llu bytes, data has room for %llu", who, (unsigned long long)total, (unsigned long long)data_cap);
  const size_t out_bytes = up256((size_t)total + 8);
  if (cnt_bytes + offs_bytes + scan_bytes + out_bytes > e->ws_limit) return over_limit(e, who, cnt_bytes + offs_bytes + scan_bytes + out_bytes);
  if ((rc = ensure(e, e->sp_temp, out_bytes)) != TAD_OK) return rc;
  uint8_t *packed = static_cast<uint8_t *>(e->sp_temp.p);
  launch_sd_export(s, d->recs, d->arena, first_code, n_values, off, packed);
  HIP_TRY(e, hipMemcpyAsync(offsets, off, (n_values + 1) * 8, hipMemcpyDeviceToHost, s));
  if (total) HIP_TRY(e, hipMemcpyAsync(data, packed, total, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  return TAD_OK;
}

int tad_strdict_import(tad_engine *eng, tad_strdict *d, uint64_t n_values, const int64_t *offsets, const uint8_t *data) {
  const char *who = "tad_strdict_import";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (n_values && !offsets) || n_values > kSdMaxValues) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (fewer than 2^32 - 1 values)", who);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  if (d->K != 0) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the dictionary holds %llu values (import fills an empty one)", who, (unsigned long long)d->K);
  if (n_values == 0) return TAD_OK;
  if (offsets[0] != 0) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: offsets[0] = %lld (the offsets start at 0)", who, (long long)offsets[0]);
  for (uint64_t i = 0; i < n_values; ++i)
    if (offsets[i + 1] < offsets[i]) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: offsets decrease at value %llu", who, (unsigned long long)i);
  if (offsets[n_values] != 0 && !data) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: data is NULL", who);
  std::vector<int64_t> codes;
  try { codes.resize(n_values); } catch (...) { return fail(eng, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  tad_string_column col{};
  col.n_rows = n_values; col.offsets = offsets; col.offset_bits = 64; col.data = data; col.data_bytes = (uint64_t)offsets[n_values]; col.memory = TAD_MEM_HOST;
  // encode on the empty dictionary; every row must be a new value, so two equal strings are found before anything is appended
  return sd_run(eng, d, &col, codes.data(), nullptr, 0, nullptr, nullptr, true, n_values, who);
}

// tad.h: a value mask from the dictionary's strings (kernel: k_sd_match).  The dictionary is only read.
int tad_strdict_match(tad_engine *eng, const tad_strdict *d, int32_t op, const uint8_t *pattern, uint64_t pattern_len, uint8_t *mask, uint64_t mask_len, tad_mem memory,
                      uint64_t *n_matched) {
  const char *who = "tad_strdict_match";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (op != TAD_STR_EQUAL && op != TAD_STR_CONTAINS_NOCASE) || pattern_len > kSdMaxPattern || (pattern_len && !pattern) || (mask_len && !mask) ||
      (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, op TAD_STR_EQUAL / TAD_STR_CONTAINS_NOCASE, a pattern of at most %u bytes, mask in host or device memory)",
                who, kSdMaxPattern);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  if (mask_len != K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: mask has %llu entries, the dictionary holds %llu values", who, (unsigned long long)mask_len, (unsigned long long)K);
  if (n_matched) *n_matched = 0;
  if (K == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  // scratch: sp_comp_a = the match count | the pattern; a host mask in in_key2
  const size_t need = 256 + up256(kSdMaxPattern) + (host ? up256(K) : 0);
  if (need > e->ws_limit) return over_limit(e, who, need);
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, 256 + up256(kSdMaxPattern))) != TAD_OK || (host && (rc = ensure(e, e->in_key2, up256(K))) != TAD_OK)) return rc;
  unsigned long long *n_hit_dev = static_cast<unsigned long long *>(e->sp_comp_a.p);
  uint8_t *pat_dev = static_cast<uint8_t *>(e->sp_comp_a.p) + 256;
  uint8_t folded[kSdMaxPattern];
  for (uint64_t i = 0; i < pattern_len; ++i) {
    const uint8_t c = pattern[i];
    folded[i] = op == TAD_STR_CONTAINS_NOCASE && c >= 'A' && c <= 'Z' ? (uint8_t)(c + 32) : c;
  }
  HIP_TRY(e, hipMemsetAsync(n_hit_dev, 0, 8, s));
  if (pattern_len) HIP_TRY(e, hipMemcpyAsync(pat_dev, folded, pattern_len, hipMemcpyHostToDevice, s));
  uint8_t *d_mask = host ? static_cast<uint8_t *>(e->in_key2.p) : mask;
  launch_sd_match(s, d->recs, d->arena, K, op, pat_dev, (uint32_t)pattern_len, d_mask, n_hit_dev);
  unsigned long long n_hit = 0;
  HIP_TRY(e, hipMemcpyAsync(&n_hit, n_hit_dev, 8, hipMemcpyDeviceToHost, s));
  if (host) HIP_TRY(e, hipMemcpyAsync(mask, d_mask, K, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (n_matched) *n_matched = n_hit;
  return TAD_OK;
}

// tad.h: a value mask from a LIKE pattern with % and _ (tad_like.h: the pattern is compiled here, on the host; kernel: k_sd_like).  The
// dictionary is only read.
int tad_strdict_like(tad_engine *eng, const tad_strdict *d, const uint8_t *pattern, uint64_t pattern_len, uint32_t flags, uint8_t *mask, uint64_t mask_len,
                     tad_mem memory, uint64_t *n_matched) {
  const char *who = "tad_strdict_like";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (flags & ~TAD_LIKE_NOCASE) != 0u || pattern_len > kSdMaxPattern || (pattern_len && !pattern) || (mask_len && !mask) ||
      (memory != TAD_MEM_HOST && memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, flags TAD_LIKE_NOCASE or 0, a pattern of at most %u bytes, mask in host or device memory)", who,
                kSdMaxPattern);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  if (mask_len != K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: mask has %llu entries, the dictionary holds %llu values", who, (unsigned long long)mask_len, (unsigned long long)K);
  if (n_matched) *n_matched = 0;
  if (K == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = memory == TAD_MEM_HOST;
  // scratch: sp_comp_a = the match count | the token program; a host mask in in_key2
  const size_t prog_bytes = up256(kLikeMaxTokens * sizeof(uint16_t));
  const size_t need = 256 + prog_bytes + (host ? up256(K) : 0);
  if (need > e->ws_limit) return over_limit(e, who, need);
  int rc;
  if ((rc = ensure(e, e->sp_comp_a, 256 + prog_bytes)) != TAD_OK || (host && (rc = ensure(e, e->in_key2, up256(K))) != TAD_OK)) return rc;
  unsigned long long *n_hit_dev = static_cast<unsigned long long *>(e->sp_comp_a.p);
  uint16_t *prog_dev = reinterpret_cast<uint16_t *>(static_cast<uint8_t *>(e->sp_comp_a.p) + 256);
  uint16_t prog[kLikeMaxTokens];
  uint32_t min_len = 0;
  const uint32_t n_tok = like_compile(pattern, (uint32_t)pattern_len, flags, prog, &min_len);
  HIP_TRY(e, hipMemsetAsync(n_hit_dev, 0, 8, s));
  if (n_tok) HIP_TRY(e, hipMemcpyAsync(prog_dev, prog, n_tok * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  uint8_t *d_mask = host ? static_cast<uint8_t *>(e->in_key2.p) : mask;
  launch_sd_like(s, d->recs, d->arena, K, prog_dev, n_tok, min_len, (flags & TAD_LIKE_NOCASE) != 0u, d_mask, n_hit_dev);
  unsigned long long n_hit = 0;
  HIP_TRY(e, hipMemcpyAsync(&n_hit, n_hit_dev, 8, hipMemcpyDeviceToHost, s));
  if (host) HIP_TRY(e, hipMemcpyAsync(mask, d_mask, K, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (n_matched) *n_matched = n_hit;
  return TAD_OK;
}

// tad.h: codes -> strings in Arrow's layout (kernels: k_sd_decode_lens, the scan, k_sd_decode).  The dictionary is only read.
int tad_strdict_decode(tad_engine *eng, const tad_strdict *d, const int64_t *codes, uint64_t n, tad_mem codes_memory, int64_t *offsets, uint8_t *data,
                       uint64_t data_cap, tad_mem out_memory, uint64_t *data_bytes) {
  const char *who = "tad_strdict_decode";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (n && !codes) || (!offsets && data) || (data_cap && !data) || (codes_memory != TAD_MEM_HOST && codes_memory != TAD_MEM_DEVICE) ||
      (out_memory != TAD_MEM_HOST && out_memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, codes, offsets with data, host or device memory)", who);
  if (n >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %llu codes do not fit 32-bit row indices", who, (unsigned long long)n);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const bool query = !offsets && !data, host_codes = codes_memory == TAD_MEM_HOST, host_out = out_memory == TAD_MEM_HOST;
  if (n == 0 && (query || host_out)) {
    if (data_bytes) *data_bytes = 0;
    if (offsets) offsets[0] = 0;
    return TAD_OK;
  }
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  if (n == 0) {      // offsets[0] = 0 in device memory
    if (data_bytes) *data_bytes = 0;
    HIP_TRY(e, hipMemsetAsync(offsets, 0, 8, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return TAD_OK;
  }
  // scratch: sp_val_a = flag word | a host call's codes | lengths | offsets (sd_decode_layout), scan_scratch; sp_temp = a host call's packed bytes
  Carve measure(nullptr);
  sd_decode_layout(measure, n, host_codes);
  const size_t scan_bytes = scan_scratch_elems(n) * sizeof(unsigned long long);
  if (measure.bytes() + scan_bytes > e->ws_limit) return over_limit(e, who, measure.bytes() + scan_bytes);
  int rc;
  if ((rc = ensure(e, e->sp_val_a, measure.bytes())) != TAD_OK || (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK) return rc;
  Carve place(e->sp_val_a.p);
  const SdDecodeWs w = sd_decode_layout(place, n, host_codes);
  const long long *d_codes = reinterpret_cast<const long long *>(codes);
  HIP_TRY(e, hipMemsetAsync(w.flags, 0, 4, s));
  if (host_codes) {
    HIP_TRY(e, hipMemcpyAsync(w.codes, codes, n * 8, hipMemcpyHostToDevice, s));
    d_codes = w.codes;
  }
  // 1. the lengths (every code is checked here) and their scan: the offsets, and the bytes needed behind them
  launch_sd_decode_lens(s, d->recs, d->K, d_codes, n, w.cnt, w.flags);
  launch_scan(s, w.cnt, w.off, n, static_cast<unsigned long long *>(e->scan_scratch.p));
  unsigned long long total = 0;
  uint32_t flags = 0;
  HIP_TRY(e, hipMemcpyAsync(&total, w.off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&flags, w.flags, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (flags & SD_FLAG_BAD_CODE)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: a code lies outside the %llu values held (TAD_CODE_NONE is no value; nothing written)", who, (unsigned long long)d->K);
  if (data_bytes) *data_bytes = total;
  if (query) return TAD_OK;
  if (total > data_cap)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: the values hold %llu bytes, data has room for %llu", who, (unsigned long long)total, (unsigned long long)data_cap);
  // 2. the bytes, straight into device `data` (any alignment) or into sp_temp on their way to the host
  uint8_t *d_data = data;
  if (host_out && total) {
    const size_t out_bytes = up256((size_t)total);
    if (measure.bytes() + scan_bytes + out_bytes > e->ws_limit) return over_limit(e, who, measure.bytes() + scan_bytes + out_bytes);
    if ((rc = ensure(e, e->sp_temp, out_bytes)) != TAD_OK) return rc;
    d_data = static_cast<uint8_t *>(e->sp_temp.p);
  }
  if (total) launch_sd_decode(s, d->recs, d->arena, d_codes, n, w.off, d_data);
  HIP_TRY(e, hipMemcpyAsync(offsets, w.off, (n + 1) * 8, host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  if (host_out && total) HIP_TRY(e, hipMemcpyAsync(data, d_data, total, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  return TAD_OK;
}

// tad.h: values leave, the survivors are renumbered densely and the arena is packed (kernels: k_sd_compact_*, two scans).  Fresh records,
// a fresh arena and a fresh table are filled beside the dictionary's and swapped in together once every launch has succeeded.
int tad_strdict_compact(tad_engine *eng, tad_strdict *d, const uint8_t *keep, uint64_t keep_len, tad_mem keep_memory, int64_t *remap, tad_mem remap_memory,
                        tad_strdict_compact_stats *stats) {
  const char *who = "tad_strdict_compact";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!d || (keep_len && (!keep || !remap)) || (keep_memory != TAD_MEM_HOST && keep_memory != TAD_MEM_DEVICE) ||
      (remap_memory != TAD_MEM_HOST && remap_memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments (dictionary, keep and remap of num_values entries in host or device memory); dictionary unchanged", who);
  std::lock_guard<std::mutex> dict_lk(d->mu);
  const uint64_t K = d->K;
  if (keep_len != K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: keep has %llu entries, the dictionary holds %llu values (dictionary unchanged)", who, (unsigned long long)keep_len,
                (unsigned long long)K);
  tad_strdict_compact_stats cs{};
  cs.values_before = cs.values_after = K;
  cs.bytes_before = cs.bytes_after = d->slots * 8 + d->rec_cap * 16 + d->arena_cap;
  cs.arena_used_before = cs.arena_used_after = d->arena_used;
  cs.job_context = -1;
  if (K == 0) {
    if (stats) *stats = cs;
    return TAD_OK;
  }
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  cs.job_context = e->index;
  const bool host_keep = keep_memory == TAD_MEM_HOST, host_remap = remap_memory == TAD_MEM_HOST;
  // scratch: sp_val_a = the block of sd_compact_layout, scan_scratch
  Carve measure(nullptr);
  sd_compact_layout(measure, K, host_keep, host_remap);
  const size_t scan_bytes = scan_scratch_elems(K) * sizeof(unsigned long long);
  if (measure.bytes() + scan_bytes > e->ws_limit) return over_limit(e, who, measure.bytes() + scan_bytes, " (dictionary unchanged)");
  int rc;
  if ((rc = ensure(e, e->sp_val_a, measure.bytes())) != TAD_OK || (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK) return rc;
  Carve place(e->sp_val_a.p);
  const SdCompactWs w = sd_compact_layout(place, K, host_keep, host_remap);
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const uint8_t *d_keep = keep;
  long long *d_remap = host_remap ? w.remap : reinterpret_cast<long long *>(remap);
  // 1. who survives, what it takes; the new codes and the new arena offsets; one round trip for the two totals
  HIP_TRY(e, hipEventRecord(e->ev[0], s));
  if (host_keep) {
    HIP_TRY(e, hipMemcpyAsync(w.keep, keep, K, hipMemcpyHostToDevice, s));
    d_keep = w.keep;
  }
  launch_sd_compact_flags(s, d_keep, d->recs, K, w.live, w.units);
  launch_scan(s, w.live, w.newcode, K, scratch);
  launch_scan(s, w.units, w.off16, K, scratch);
  unsigned long long m = 0, units = 0;
  HIP_TRY(e, hipMemcpyAsync(&m, w.newcode + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&units, w.off16 + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  const uint64_t bytes = units * 16ull;
  if (m > K || bytes > d->arena_used)
    return fail(e, TAD_ERR_HIP, "%s: %llu survivors of %llu values, %llu of %llu bytes; dictionary unchanged", who, (unsigned long long)m, (unsigned long long)K,
                (unsigned long long)bytes, (unsigned long long)d->arena_used);
  auto remap_out = [&](hipError_t r) -> hipError_t {
    if (r == hipSuccess && host_remap) r = hipMemcpyAsync(remap, d_remap, K * 8, hipMemcpyDeviceToHost, s);
    if (r == hipSuccess) r = hipEventRecord(e->ev[1], s);
    r = finish_stream(e, r);
    if (r == hipSuccess) r = hipEventElapsedTime(&cs.ms_total, e->ev[0], e->ev[1]);
    return r;
  };
  if (m == K) {      // nothing retired: the identity, the dictionary as it is
    launch_sd_compact_recs(s, w.live, w.newcode, w.off16, d->recs, K, d_remap, nullptr, nullptr);
    const hipError_t r = remap_out(hipSuccess);
    if (r != hipSuccess) return fail(e, TAD_ERR_HIP, "%s: %s (dictionary unchanged)", who, hipGetErrorString(r));
    if (stats) *stats = cs;
    return TAD_OK;
  }
  // 2. fresh records, arena and table at the size tad_strdict_create(2 m, twice the survivors' bytes) picks — its minimum for m == 0 —
  //    and never above the current one
  uint64_t ncap = 2 * m > kSdMinValues ? 2 * m : kSdMinValues, nslots = pow2_at_least(4 * m), narena_cap = bytes ? 2 * bytes : 16;
  if (ncap > d->rec_cap) ncap = d->rec_cap;
  if (nslots > d->slots) nslots = d->slots;
  if (narena_cap > d->arena_cap) narena_cap = d->arena_cap;
  Candidate<void> nrecs;
  Candidate<uint8_t> narena;
  Candidate<unsigned long long> ntable;
  hipError_t r = nrecs.alloc(e, ncap, ncap * 16);
  if (r == hipSuccess) r = narena.alloc(e, narena_cap, narena_cap);
  if (r == hipSuccess) r = ntable.alloc(e, nslots, nslots * 8);
  if (r == hipSuccess) r = hipMemsetAsync(ntable.p, 0xFF, nslots * 8, s);
  // 3. remap and the survivors' records; their bytes; their slots
  if (r == hipSuccess) {
    launch_sd_compact_recs(s, w.live, w.newcode, w.off16, d->recs, K, d_remap, nrecs.p, w.src16);
    launch_sd_compact_copy(s, nrecs.p, w.src16, m, d->arena, narena.p);
    if (m) launch_sd_compact_rehash(s, d->table, d->slots, d->recs, K, d_remap, ntable.p, nslots);
  }
  r = remap_out(r);
  if (r != hipSuccess) (void)hipGetLastError();
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP, "%s: %s (dictionary unchanged)", who, hipGetErrorString(r));
  nrecs.commit_into(d->recs, d->rec_cap);
  narena.commit_into(d->arena, d->arena_cap);
  ntable.commit_into(d->table, d->slots);
  d->K = m;
  d->arena_used = bytes;
  cs.values_after = m;
  cs.bytes_after = d->slots * 8 + d->rec_cap * 16 + d->arena_cap;
  cs.arena_used_after = bytes;
  if (stats) *stats = cs;
  return TAD_OK;
}

}  // extern "C"
