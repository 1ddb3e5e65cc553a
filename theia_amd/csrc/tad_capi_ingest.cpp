// tad_capi_ingest.cpp — the ingest entry points of include/tad.h: rows bucketed by owner for the all-to-all(v),
// key tuples -> dense ids, Arrow string columns -> dictionary codes, Arrow buffers -> 8-byte device columns, row masks, the synthetic table,
// flow rows -> the drop job's rows.
#include "tad_capi_dict.h"

using namespace tad;
using namespace tadh;

extern "C" {

int tad_shard_rows(tad_engine *eng, const tad_columns *cols, uint32_t world, uint64_t *out_key_id, int64_t *out_flow_end_s,
                   uint64_t *out_value, uint64_t *counts) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_shard_rows: engine is NULL");
  if (!cols || !counts || !shard_world_ok(world)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_shard_rows: bad arguments (1 <= world <= 1024)");
  if (cols->memory != TAD_MEM_DEVICE || cols->key_id2 || cols->flow_start_s)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_shard_rows: device columns with one key per row only");
  const uint64_t n = cols->n_rows;
  if (n && (!cols->key_id || !cols->flow_end_s || !cols->value || !out_key_id || !out_flow_end_s || !out_value))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_shard_rows: key_id, flow_end_s, value and the three outputs are required");
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_shard_rows: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int rc;
  if ((rc = ensure(e, e->scan_scratch, (size_t)world * 16)) != TAD_OK) return rc;
  unsigned long long *d_counts = static_cast<unsigned long long *>(e->scan_scratch.p);
  unsigned long long *d_cursor = d_counts + world;
  HIP_TRY(e, hipMemsetAsync(d_counts, 0, (size_t)world * 8, s));
  launch_shard_count(s, cols->key_id, n, world, d_counts);
  std::vector<unsigned long long> h(world), off(world);
  HIP_TRY(e, hipMemcpyAsync(h.data(), d_counts, (size_t)world * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  unsigned long long run = 0;
  for (uint32_t d = 0; d < world; ++d) { off[d] = run; run += h[d]; counts[d] = h[d]; }
  HIP_TRY(e, hipMemcpyAsync(d_cursor, off.data(), (size_t)world * 8, hipMemcpyHostToDevice, s));
  launch_shard_scatter(s, cols->key_id, cols->flow_end_s, cols->value, n, world, d_cursor, out_key_id, out_flow_end_s, out_value);
  HIP_TRY(e, hipStreamSynchronize(s));   // `off` goes out of scope; the caller may hand the buffers to a collective on another stream
  HIP_TRY(e, hipGetLastError());
  return TAD_OK;
}

}  // extern "C"

// tad_factorize / tad_factorize_hist
static int factorize_impl(tad_engine *eng, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *first_row, uint64_t first_row_cap,
                          uint64_t *num_keys, tad_key_hist *hist) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_factorize: engine is NULL");
  if (!kc || !num_keys || kc->n_cols < 1 || kc->n_cols > kFzMaxCols || !kc->cols_a || (kc->n_rows && !key_id) || (kc->cols_b && kc->n_rows && !key_id2) ||
      (first_row_cap && !first_row))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_factorize: bad arguments (1..%d key columns, key_id / key_id2 / first_row buffers)", kFzMaxCols);
  const uint64_t n = kc->n_rows;
  const uint32_t sides = kc->cols_b ? 2 : 1;
  *num_keys = 0;
  uint32_t *hist_bins = nullptr;
  PartPlan hpl{};
  if (hist != nullptr) {
    hist_bins = hist->bins;
    hist->n_rows = hist->num_keys = hist->chunk_rows = 0;
    hist->workgroups = hist->nbins = hist->shift = hist->sides = 0;
    // pass B's row chunking does not depend on the key count (part_plan_bins): the kernel needs it before the count exists on the host
    if (hist_bins == nullptr || !part_plan_bins(n, 1, sides == 2, &hpl)) hist_bins = nullptr;
  }
  if (n == 0) return TAD_OK;
  if (n * sides >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_factorize: %llu virtual rows do not fit 32-bit row indices", (unsigned long long)(n * sides));
  for (int c = 0; c < kc->n_cols; ++c)
    if (!kc->cols_a[c] || (kc->cols_b && !kc->cols_b[c])) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_factorize: key column %d is NULL", c);
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_factorize: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = kc->memory == TAD_MEM_HOST;
  // host inputs are staged behind the table block in the same scratch: columns, masks, outputs
  const size_t col_bytes = up256(n * 8), fr_bytes = up256(first_row_cap * 8);
  const size_t stage = host ? key_stage_bytes(kc) + sides * col_bytes + fr_bytes : 0;
  unsigned long long nk = 0;
  uint64_t *d_key = key_id, *d_key2 = key_id2, *d_fr = first_row;
  // the table starts small and grows when the device says so (tad_factorize.hip): 2^20 -> 2^24 -> 2 n slots
  int rc = with_factorize_ladder(e, n * sides, "tad_factorize", "", "table", 64, [&](size_t tb) { return tb + stage; }, [&](uint64_t slots, size_t tb, bool *grow) -> int {
    int rc;
    if ((rc = ensure(e, e->sp_temp, tb + stage + 64)) != TAD_OK) return rc;
    unsigned char *base = static_cast<unsigned char *>(e->sp_temp.p);
    unsigned long long *nk_dev = reinterpret_cast<unsigned long long *>(base + tb);
    TupleBatch A;      // (a host batch is staged again on every rung: the block may have moved)
    if ((rc = stage_key_columns(e, kc, host ? base + tb + 64 : nullptr, &A)) != TAD_OK) return rc;
    if (host) {
      unsigned char *p = base + tb + 64 + key_stage_bytes(kc);
      d_key = reinterpret_cast<uint64_t *>(p); p += col_bytes;
      if (sides == 2) { d_key2 = reinterpret_cast<uint64_t *>(p); p += col_bytes; }
      d_fr = reinterpret_cast<uint64_t *>(p);
    }
    uint32_t *flags_dev = nullptr;
    launch_factorize(s, A.a, A.keep_a, sides == 2 ? A.b : nullptr, A.keep_b, n, kc->n_cols, slots, base, d_key, d_key2, d_fr, first_row_cap, nk_dev, &flags_dev,
                     hist_bins, hpl.G, hpl.chunk);
    uint32_t flags = 0;
    HIP_TRY(e, hipMemcpyAsync(&nk, nk_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    *grow = flags != 0;      // more keys than this table takes
    return TAD_OK;
  });
  if (rc != TAD_OK) return rc;
  if (host) {
    HIP_TRY(e, hipMemcpyAsync(key_id, d_key, n * 8, hipMemcpyDeviceToHost, s));
    if (sides == 2) HIP_TRY(e, hipMemcpyAsync(key_id2, d_key2, n * 8, hipMemcpyDeviceToHost, s));
    const uint64_t m = nk < first_row_cap ? nk : first_row_cap;
    if (m) HIP_TRY(e, hipMemcpyAsync(first_row, d_fr, m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
  }
  *num_keys = nk;
  if (hist_bins != nullptr && nk != 0 && part_plan_bins(n, nk, sides == 2, &hpl)) {   // what the kernel derived from the device-side count
    hist->n_rows = n; hist->num_keys = nk; hist->chunk_rows = hpl.chunk;
    hist->workgroups = (uint32_t)hpl.G; hist->nbins = hpl.nbins; hist->shift = (uint32_t)hpl.shift_bin; hist->sides = sides;
  }
  return TAD_OK;
}

extern "C" {

int tad_factorize(tad_engine *eng, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *first_row, uint64_t first_row_cap,
                  uint64_t *num_keys) {
  return factorize_impl(eng, kc, key_id, key_id2, first_row, first_row_cap, num_keys, nullptr);
}

int tad_factorize_hist(tad_engine *eng, const tad_key_columns *kc, uint64_t *key_id, uint64_t *key_id2, uint64_t *first_row, uint64_t first_row_cap,
                       uint64_t *num_keys, tad_key_hist *hist) {
  if (eng && !hist) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_factorize_hist: hist is NULL");
  return factorize_impl(eng, kc, key_id, key_id2, first_row, first_row_cap, num_keys, hist);
}

int tad_encode_strings(tad_engine *eng, const tad_string_column *col, int64_t *codes, uint64_t *first_row, uint64_t first_row_cap, uint64_t *num_values) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_encode_strings: engine is NULL");
  if (!col || !num_values || (col->offset_bits != 32 && col->offset_bits != 64) || (col->n_rows && (!col->offsets || !codes)) || (first_row_cap && !first_row) ||
      (col->data_bytes && !col->data))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_encode_strings: bad arguments (offsets of 32 or 64 bits, data, codes / first_row buffers)");
  const uint64_t n = col->n_rows;
  *num_values = 0;
  if (n == 0) return TAD_OK;
  if (n >= 0xFFFFFFFFull) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_encode_strings: %llu rows do not fit 32-bit row indices", (unsigned long long)n);
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_encode_strings: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = col->memory == TAD_MEM_HOST;
  // host inputs are staged behind the table block: offsets, bytes (+ 8 of slack: the last aligned word), validity, codes, first rows
  const size_t code_bytes = up256(n * 8), fr_bytes = up256(first_row_cap * 8);
  const size_t stage = host ? string_stage_bytes(col, 8) + code_bytes + fr_bytes : 0;
  unsigned long long nv = 0;
  long long *d_codes = reinterpret_cast<long long *>(codes);
  uint64_t *d_fr = first_row;
  // more distinct values than a table takes: once more with the next size (2^20 -> 2^24 -> 2 n slots)
  int rc = with_factorize_ladder(e, n, "tad_encode_strings", "", "table", 64, [&](size_t tb) { return tb + stage; }, [&](uint64_t slots, size_t tb, bool *grow) -> int {
    int rc;
    if ((rc = ensure(e, e->sp_temp, tb + stage + 64)) != TAD_OK) return rc;
    unsigned char *base = static_cast<unsigned char *>(e->sp_temp.p);
    unsigned long long *nv_dev = reinterpret_cast<unsigned long long *>(base + tb);
    StrBatch B;
    if ((rc = stage_string_column(e, col, host ? base + tb + 64 : nullptr, 8, &B)) != TAD_OK) return rc;
    if (host) {
      unsigned char *p = base + tb + 64 + string_stage_bytes(col, 8);
      d_codes = reinterpret_cast<long long *>(p); p += code_bytes;
      d_fr = reinterpret_cast<uint64_t *>(p);
    }
    uint32_t *flags_dev = nullptr;
    launch_encode_strings(s, B.off, B.off64, B.data, B.data_bytes, B.valid, B.valid_off, n, slots, base, d_codes, d_fr, first_row_cap, nv_dev, &flags_dev);
    uint32_t flags = 0;
    HIP_TRY(e, hipMemcpyAsync(&nv, nv_dev, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(&flags, flags_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    if (flags & 2u) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_encode_strings: offsets decrease or point beyond data_bytes");
    *grow = (flags & 1u) != 0;
    return TAD_OK;
  });
  if (rc != TAD_OK) return rc;
  if (host) {
    HIP_TRY(e, hipMemcpyAsync(codes, d_codes, n * 8, hipMemcpyDeviceToHost, s));
    const uint64_t m = nv < first_row_cap ? nv : first_row_cap;
    if (m) HIP_TRY(e, hipMemcpyAsync(first_row, d_fr, m * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
  }
  *num_values = nv;
  return TAD_OK;
}

int tad_synth_generate(tad_engine *eng, uint64_t seed, uint64_t first_row, uint64_t n_rows, uint64_t num_keys,
                       uint64_t n_buckets, uint64_t *key_id, int64_t *flow_end_s, uint64_t *value) {
  if (!eng || num_keys == 0 || n_buckets == 0 || (n_rows && (!key_id || !flow_end_s || !value)))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_synth_generate: bad arguments");
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_synth_generate: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  launch_synth(e->stream, seed, first_row, n_rows, num_keys, n_buckets, key_id, flow_end_s, value);
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, hipGetLastError());
  return TAD_OK;
}

// ---- columnar ingest: Arrow buffers in host memory -> 8-byte device columns ----
int tad_widen_column(tad_engine *eng, const void *src, int32_t src_bits, int32_t src_signed, tad_mem src_memory, uint64_t n, const int64_t *table,
                     uint64_t table_len, int64_t *dst) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_widen_column: engine is NULL");
  if ((src_bits != 8 && src_bits != 16 && src_bits != 32 && src_bits != 64) || (n && (!src || !dst)) || (table_len && !table))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_widen_column: bad arguments (src of 8 / 16 / 32 / 64 bits, src / dst buffers, table)");
  if (n == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_widen_column: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const size_t bytes = (size_t)n * (size_t)(src_bits / 8);
  if (src_memory == TAD_MEM_HOST && src_bits == 64 && table == nullptr) {      // nothing to convert: the copy is the column
    HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return TAD_OK;
  }
  int rc;
  if ((rc = ensure(e, e->counters, kTailBytes)) != TAD_OK) return rc;
  unsigned int *err = reinterpret_cast<unsigned int *>(e->counters.p);
  HIP_TRY(e, hipMemsetAsync(err, 0, 4, s));
  const void *d_src = src;
  if (src_memory == TAD_MEM_HOST) {
    if ((rc = ensure(e, e->in_key, bytes)) != TAD_OK) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->in_key.p, src, bytes, hipMemcpyHostToDevice, s));
    d_src = e->in_key.p;
  }
  launch_widen(s, d_src, src_bits, src_signed != 0, n, reinterpret_cast<const long long *>(table), table ? table_len : 0, reinterpret_cast<long long *>(dst), err);
  unsigned int herr = 0;
  HIP_TRY(e, hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (herr) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_widen_column: an index lies outside the table of %llu entries", (unsigned long long)table_len);
  return TAD_OK;
}

int tad_mask_rows(tad_engine *eng, uint64_t n, int32_t n_terms, const int64_t *const *codes, const uint8_t *const *masks, const uint64_t *mask_len,
                  int32_t combine, uint8_t *keep) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_mask_rows: engine is NULL");
  if (n_terms < 0 || n_terms > kMaskMaxTerms || (n_terms && (!codes || !masks || !mask_len)) || (n && !keep))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_mask_rows: bad arguments (0..%d terms, keep buffer)", kMaskMaxTerms);
  for (int t = 0; t < n_terms; ++t)
    if (n && (!codes[t] || !masks[t])) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_mask_rows: term %d is NULL", t);
  if (n == 0) return TAD_OK;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_mask_rows: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int rc;
  if ((rc = ensure(e, e->counters, kTailBytes)) != TAD_OK) return rc;
  unsigned int *err = reinterpret_cast<unsigned int *>(e->counters.p);
  HIP_TRY(e, hipMemsetAsync(err, 0, 4, s));
  launch_mask_rows(s, n, n_terms, reinterpret_cast<const long long *const *>(codes), masks, mask_len, combine != 0, keep, err);
  unsigned int herr = 0;
  HIP_TRY(e, hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (herr) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_mask_rows: a code lies outside its mask");
  return TAD_OK;
}

// ---- the drop job's flow-row query: tad_drop_select (tad_drop_select.hip) ----
int tad_drop_select(tad_engine *eng, const tad_drop_flow_columns *cols, int64_t start_time, int64_t end_time, tad_mem out_memory, tad_drop_rows **out) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: engine is NULL");
  if (!cols || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: cols / out is NULL");
  *out = nullptr;
  if ((cols->memory != TAD_MEM_HOST && cols->memory != TAD_MEM_DEVICE) || (out_memory != TAD_MEM_HOST && out_memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: memory must be TAD_MEM_HOST or TAD_MEM_DEVICE");
  if (cols->flags & ~TAD_FLAG_TIME_U32) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: flags 0x%x: only TAD_FLAG_TIME_U32 is understood", cols->flags);
  if (end_time != 0 && !cols->flow_end_s) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: end_time is set and flow_end_s is NULL");
  const uint64_t n = cols->n_rows;
  if (n && (!cols->ingress_action || !cols->egress_action || !cols->flow_start_s || !cols->src_ip || !cols->src_pod_ns || !cols->src_pod_name || !cols->dst_ip ||
            !cols->dst_pod_ns || !cols->dst_pod_name))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_drop_select: the two action columns, flow_start_s and the six code columns are required");
  DropRowsPriv *rp = new (std::nothrow) DropRowsPriv();
  if (!rp) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  memset(rp, 0, sizeof *rp);
  rp->pub.memory = out_memory;
  if (n == 0) { *out = &rp->pub; return TAD_OK; }
  struct Guard { DropRowsPriv *p; ~Guard() { delete p; } } guard{rp};   // (until the result is handed over)
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_drop_select: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const bool host = cols->memory == TAD_MEM_HOST;
  const int t32 = (cols->flags & TAD_FLAG_TIME_U32) ? 1 : 0;
  const uint64_t tiles = dsel_tiles(n);
  // workspace: row bitmask | tile counts | tile offsets (64-bit) | scan scratch | total | a host table's columns
  const DselDims dims{n, (n + kDselLaneRows - 1) / kDselLaneRows, tiles, scan_scratch_elems(tiles), t32 != 0, host, cols->flow_end_s != nullptr, cols->keep != nullptr};
  const size_t need = carved_bytes(dsel_layout, dims);
  if (need > e->ws_limit) return over_limit(e, "tad_drop_select", need);
  int rc;
  DselWs ws;
  if ((rc = carve_buf(e, e->dsel, &ws, dsel_layout, dims)) != TAD_OK) return rc;
  uint16_t *bits = ws.bits;
  uint32_t *cnt = ws.cnt;
  unsigned long long *off = ws.off, *scratch = ws.scratch, *total_dev = ws.total;
  DselIn A{};
  A.ia = cols->ingress_action; A.ea = cols->egress_action; A.keep = cols->keep;
  A.ts = cols->flow_start_s; A.te = cols->flow_end_s;
  const int64_t *codes[6] = {cols->src_ip, cols->src_pod_ns, cols->src_pod_name, cols->dst_ip, cols->dst_pod_ns, cols->dst_pod_name};
  if (host) {
    auto put = [&](void *dst, const void *src, size_t bytes) -> const void * {
      return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess ? dst : nullptr;
    };
    bool ok = true;
    ok = ok && (A.ia = static_cast<const uint8_t *>(put(ws.ia, cols->ingress_action, n))) != nullptr;
    ok = ok && (A.ea = static_cast<const uint8_t *>(put(ws.ea, cols->egress_action, n))) != nullptr;
    ok = ok && (A.ts = put(ws.ts, cols->flow_start_s, (size_t)n * (t32 ? 4 : 8))) != nullptr;
    if (cols->flow_end_s) ok = ok && (A.te = put(ws.te, cols->flow_end_s, (size_t)n * (t32 ? 4 : 8))) != nullptr;
    for (int c = 0; c < 6; ++c) ok = ok && (codes[c] = static_cast<const int64_t *>(put(ws.codes[c], codes[c], (size_t)n * 8))) != nullptr;
    if (cols->keep) ok = ok && (A.keep = static_cast<const uint8_t *>(put(ws.keep, cols->keep, n))) != nullptr;
    if (!ok) { (void)hipGetLastError(); return fail(e, TAD_ERR_HIP, "tad_drop_select: staging the host columns failed"); }
  }
  A.src_ip = reinterpret_cast<const long long *>(codes[0]); A.src_ns = reinterpret_cast<const long long *>(codes[1]); A.src_pod = reinterpret_cast<const long long *>(codes[2]);
  A.dst_ip = reinterpret_cast<const long long *>(codes[3]); A.dst_ns = reinterpret_cast<const long long *>(codes[4]); A.dst_pod = reinterpret_cast<const long long *>(codes[5]);
  A.src_null = cols->src_pod_null; A.dst_null = cols->dst_pod_null;
  A.start_time = start_time; A.end_time = end_time;
  A.n = n; A.t32 = t32;
  launch_dsel_flags(s, A, bits, cnt);
  launch_scan(s, cnt, off, tiles, scratch, total_dev);
  unsigned long long m = 0;
  HIP_TRY(e, hipMemcpyAsync(&m, total_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));     // the host sizes the result
  HIP_TRY(e, hipGetLastError());
  if (m > n) return fail(e, TAD_ERR_HIP, "tad_drop_select: internal error: %llu rows selected out of %llu", m, (unsigned long long)n);
  if (m == 0) { guard.p = nullptr; *out = &rp->pub; return TAD_OK; }
  const size_t bytes = carved_bytes(drop_rows_layout, m);
  ResultBlock blk;
  DselOut O;
  if ((rc = carve_block(e, &blk, &O, drop_rows_layout, m)) != TAD_OK) return rc;
  launch_dsel_emit(s, A, bits, off, O);
  void *h = nullptr;
  hipError_t hr = hipSuccess;
  if (out_memory == TAD_MEM_HOST) {
    h = malloc(bytes);
    if (!h) { (void)hipStreamSynchronize(s); release_block(e, blk.base, blk.cap); return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory for %zu bytes of drop rows", bytes); }
    hr = hipMemcpyAsync(h, blk.base, bytes, hipMemcpyDeviceToHost, s);
  }
  const hipError_t hs = hipStreamSynchronize(s);
  if (hr == hipSuccess) hr = hs;
  if (hr == hipSuccess) hr = hipGetLastError();
  if (hr != hipSuccess) {
    release_block(e, blk.base, blk.cap);
    free(h);
    return fail(e, TAD_ERR_HIP, "tad_drop_select: %s", hipGetErrorString(hr));
  }
  if (out_memory == TAD_MEM_HOST) {
    release_block(e, blk.base, blk.cap);
    O = carve_at(h, drop_rows_layout, m);
    rp->block = h; rp->block_cap = bytes;
  } else {
    rp->block = blk.base; rp->block_cap = blk.cap;
  }
  rp->pub.n_rows = m;
  rp->pub.endpoint_kind = reinterpret_cast<int64_t *>(O.kind);
  rp->pub.endpoint_ns = reinterpret_cast<int64_t *>(O.ns);
  rp->pub.endpoint_name = reinterpret_cast<int64_t *>(O.name);
  rp->pub.direction = reinterpret_cast<int64_t *>(O.dir);
  rp->pub.day_s = reinterpret_cast<int64_t *>(O.day);
  rp->pub.count = reinterpret_cast<uint64_t *>(O.count);
  rp->pub.row = reinterpret_cast<uint64_t *>(O.row);
  guard.p = nullptr;
  *out = &rp->pub;
  return TAD_OK;
}

void tad_drop_rows_free(tad_engine *e, tad_drop_rows *r) {
  if (!r) return;
  DropRowsPriv *rp = reinterpret_cast<DropRowsPriv *>(r);
  if (rp->block) {
    if (r->memory == TAD_MEM_DEVICE && e) release_block(e, rp->block, rp->block_cap);
    else if (r->memory == TAD_MEM_DEVICE) hipFree(rp->block);
    else free(rp->block);
  }
  delete rp;
}

}  // extern "C"
