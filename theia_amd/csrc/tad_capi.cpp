// tad_capi.cpp — what the entry points of include/tad.h share (key buffers, the rows result and its epilogue, the moments' merge), the batches
// on a streaming state that the job's count pass runs (history, series, merge, replace, ARIMA, DROP), and the calls that feed the job such a
// batch: tad_drop_stream, tad_state_merge, tad_state_replace.  The batch job itself (run_job_locked: lattice, Stage 0, count, retries) is tad_capi_job.cpp;
// the read-only jobs on a state (tad_run_state, tad_run_state_window, tad_drop_state, their *_keys forms) are tad_capi_view.cpp; the life
// of a tad_state is tad_capi_state.cpp.
#include "tad_engine.h"

using namespace tad;
using namespace tadh;

namespace tadh {

// reciprocals of the point counts 1..T for the exact-division FMA sequence (tad_internal.h:div_by_count);
// 1.0 / n on the host is IEEE division = the correctly rounded reciprocal the sequence needs.
int ensure_rcp_table(JobCtx *e, uint64_t T) {
  const uint64_t want = T + 2;
  if (want <= e->rcp_n) return TAD_OK;
  uint64_t cap = want < 1024 ? 1024 : want + want / 4;
  int rc = ensure(e, e->rcp_table, cap * sizeof(double));
  if (rc != TAD_OK) return rc;
  std::vector<double> h(cap);
  h[0] = 0.0;
  for (uint64_t i = 1; i < cap; ++i) h[i] = 1.0 / (double)i;
  HIP_TRY(e, hipMemcpyAsync(e->rcp_table.p, h.data(), cap * sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // h goes out of scope
  e->rcp_n = cap;
  return TAD_OK;
}

int ensure_key_buffers(JobCtx *e, uint64_t K) {
  int rc;
  const uint64_t k = K ? K : 1;
  if ((rc = ensure(e, e->sigma, k * sizeof(double))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->n_pts, k * sizeof(uint32_t))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->n_anom, k * sizeof(uint32_t))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->off, (k + 1) * sizeof(unsigned long long))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(k) * sizeof(unsigned long long))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->key_mean, k * sizeof(double))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->key_m2, k * sizeof(double))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->counters, kTailBytes)) != TAD_OK) return rc;
  return TAD_OK;
}

void emit_rows(JobCtx *e, Grid g, Lattice L, const JobParams &jp, OutRows out, uint64_t rows) {
  const int kind = jp.algo == TAD_ALGO_EWMA ? 0 : (jp.algo == TAD_ALGO_ARIMA ? 1 : (jp.algo == TAD_ALGO_DROP ? 3 : (jp.lazy_sigma ? 4 : 2)));
  // DBSCAN job: only keys of the detector's work list (still in e->aux) can have rows
  if (kind == 4 && !jp.all_points &&
      launch_emit_dbscan_list(e->stream, g, L, e->aux.p, static_cast<const uint32_t *>(e->n_anom.p), static_cast<const unsigned long long *>(e->off.p), out))
    return;
  launch_emit(e->stream, g, L, kind, jp.all_points, jp.alpha, static_cast<const double *>(e->sigma.p),
              static_cast<const uint32_t *>(e->n_pts.p), static_cast<const double *>(kind == 3 ? e->key_mean.p : e->calc.p),
              static_cast<const unsigned long long *>(e->off.p), out, rows, e->plan.ewma_emit, e->plan.ewma_emit_rows);
}

int make_result(JobCtx *e, uint64_t rows, bool with_anomaly, tad_mem out_memory, ResultPriv **out, OutRows *dev_rows,
                ResultBlock *dev_block) {
  ResultPriv *rp = new (std::nothrow) ResultPriv();
  if (!rp) return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  memset(rp, 0, sizeof *rp);
  const int rc = carve_block(e, dev_block, dev_rows, result_layout, rows, with_anomaly);
  if (rc != TAD_OK) { delete rp; return rc; }
  rp->pub.n_rows = rows;
  rp->pub.memory = out_memory;
  *out = rp;
  return TAD_OK;
}

// after emit: hand the device block to the caller, or copy it to a host block
int finish_result(JobCtx *e, ResultPriv *rp, uint64_t rows, bool with_anomaly, ResultBlock dev_block, OutRows dev_rows) {
  if (rp->pub.memory == TAD_MEM_DEVICE) {
    rp->block = dev_block.base;
    rp->block_cap = dev_block.cap;
    rp->pub.key_id = reinterpret_cast<uint64_t *>(dev_rows.key_id);
    rp->pub.flow_end_s = reinterpret_cast<int64_t *>(dev_rows.flow_end_s);
    rp->pub.throughput = dev_rows.throughput;
    rp->pub.algo_calc = dev_rows.algo_calc;
    rp->pub.stddev = dev_rows.stddev;
    rp->pub.anomaly = dev_rows.anomaly;
    return TAD_OK;
  }
  const size_t bytes = carved_bytes(result_layout, rows, with_anomaly);
  void *h = malloc(bytes);
  if (!h) { release_block(e, dev_block.base, dev_block.cap); return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory for %zu result bytes", bytes); }
  hipError_t r = hipMemcpyAsync(h, dev_block.base, bytes, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  release_block(e, dev_block.base, dev_block.cap);
  if (r != hipSuccess) { free(h); return fail(e, TAD_ERR_HIP, "result copy failed: %s", hipGetErrorString(r)); }
  const OutRows ho = carve_at(h, result_layout, rows, with_anomaly);
  rp->block = h;
  rp->block_cap = bytes;
  rp->pub.key_id = reinterpret_cast<uint64_t *>(ho.key_id);
  rp->pub.flow_end_s = reinterpret_cast<int64_t *>(ho.flow_end_s);
  rp->pub.throughput = ho.throughput;
  rp->pub.algo_calc = ho.algo_calc;
  rp->pub.stddev = ho.stddev;
  rp->pub.anomaly = ho.anomaly;
  return TAD_OK;
}

JobParams job_params(const tad_job *job) {
  JobParams jp;
  jp.algo = job->algo;
  jp.alpha = job->ewma_alpha == 0.0 ? 0.5 : job->ewma_alpha;
  jp.eps = job->dbscan_eps == 0.0 ? 250000000.0 : job->dbscan_eps;
  jp.min_samples = job->dbscan_min_samples == 0 ? 4 : job->dbscan_min_samples;
  jp.maxiter = job->arima_maxiter == 0 ? 50 : job->arima_maxiter;
  jp.drop_nsigma = job->drop_nsigma == 0.0 ? 3.0 : job->drop_nsigma;
  jp.drop_min_samples = job->drop_min_samples == 0 ? 3 : job->drop_min_samples;
  jp.all_points = (job->flags & TAD_FLAG_EMIT_ALL_POINTS) != 0;
  return jp;
}

void merge_moments(const Moments *blocks, bool any, double *pts_mean, double *pts_m2) {
  double mn = 0.0, mean = 0.0, m2 = 0.0;   // Chan merge of the block partials, fixed order
  if (any)
    for (int b = 0; b < kMomentBlocks; ++b) {
      const Moments &p = blocks[b];
      if (p.n == 0.0) continue;
      if (mn == 0.0) { mn = p.n; mean = p.mean; m2 = p.m2; continue; }
      const double nn = mn + p.n, d = p.mean - mean;
      mean = mean + d * (p.n / nn);
      m2 = m2 + p.m2 + d * d * (mn * p.n / nn);
      mn = nn;
    }
  *pts_mean = mean;
  *pts_m2 = m2;
}

// TAD_FLAG_EMIT_ALL_POINTS: the emit kernel wrote the verdicts; they are counted on the host copy.  Frees the result when the copy fails.
static int count_verdicts(JobCtx *e, ResultPriv *rp, uint64_t rows, uint64_t *n_anomalies) {
  *n_anomalies = 0;
  if (rows == 0) return TAD_OK;
  std::vector<uint8_t> tmp;
  const uint8_t *a = rp->pub.anomaly;
  if (rp->pub.memory == TAD_MEM_DEVICE) {
    tmp.resize(rows);
    const hipError_t cr = hipMemcpy(tmp.data(), rp->pub.anomaly, rows, hipMemcpyDeviceToHost);
    if (cr != hipSuccess) { tad_result_free(e->eng, &rp->pub); return fail(e, TAD_ERR_HIP, "verdict copy failed: %s", hipGetErrorString(cr)); }
    a = tmp.data();
  }
  for (uint64_t i = 0; i < rows; ++i) *n_anomalies += a[i];
  return TAD_OK;
}

int finish_rows(JobCtx *e, const tad_job *job, RowsOut *ro, uint64_t rows, bool with_anomaly, const DevCounters &c, bool any_points) {
  hipStream_t s = e->stream;
  ResultPriv *rp = ro->rp;
  int rc;
  const hipError_t er = hipEventRecord(e->ev[4], s);
  if (er != hipSuccess) {
    release_block(e, ro->dev_block.base, ro->dev_block.cap);
    delete rp;
    return fail(e, TAD_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(er));
  }
  if ((rc = finish_result(e, rp, rows, with_anomaly, ro->dev_block, ro->dev_rows)) != TAD_OK) { delete rp; return rc; }
  hipError_t le = hipStreamSynchronize(s);
  if (le == hipSuccess) le = hipGetLastError();
  if (le != hipSuccess) { tad_result_free(e->eng, &rp->pub); return fail(e, TAD_ERR_HIP, "kernel failure: %s", hipGetErrorString(le)); }
  tad_stats &st = rp->pub.stats;
  st.n_keys = c.n_keys;
  st.keys_no_result = c.keys_no_result;
  st.kalman_steps = c.kalman_steps;
  st.arima_fits = c.arima_fits;
  st.arima_nan_fits = c.arima_nan_fits;
  merge_moments(e->moments_host, any_points, &st.pts_mean, &st.pts_m2);
  st.n_anomalies = rows;
  if (with_anomaly && (rc = count_verdicts(e, rp, rows, &st.n_anomalies)) != TAD_OK) return rc;
  st.job_context = e->index;
  st.arima_relaunches = e->arima_relaunches;
  strncpy(rp->pub.id, job->id, sizeof rp->pub.id - 1);
  return TAD_OK;
}

// The batch's new points in (key, time) order for stream_history_batch and state_merge_batch: keys in e->hs_key, times in e->hs_t, values
// and per-key offsets in *nv / *poff.  ensure_batch_points sizes the buffers both share (hs_key, hs_t, hs_sorted, the per-key counts and
// offsets of BatchKeys in hs_kcnt / hs_koff, the scan scratch).
static int ensure_batch_points(JobCtx *e, uint64_t K, uint64_t P_cap, bool sparse, BatchKeys *bk) {
  const uint64_t pc = P_cap ? P_cap : 1;
  int rc;
  if ((rc = ensure(e, e->hs_key, pc * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_t, pc * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_sorted, pc * 8)) != TAD_OK) return rc;
  if ((rc = carve_bufs(e, e->hs_koff, e->hs_kcnt, bk, batch_keys_layout, K)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > pc ? K : pc) * sizeof(unsigned long long))) != TAD_OK) return rc;
  if (!sparse && (rc = ensure(e, e->hs_val, pc * 8)) != TAD_OK) return rc;
  return TAD_OK;
}

static void batch_points(JobCtx *e, const BatchKeys &bk, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P,
                         const unsigned long long **poff, const unsigned long long **nv) {
  hipStream_t s = e->stream;
  unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
  long long *nt = static_cast<long long *>(e->hs_t.p);
  if (sparse_poff) {   // the sorted unique points of the sparse Stage 0
    *poff = sparse_poff;
    *nv = static_cast<const unsigned long long *>(e->sp_val_a.p);
    launch_hist_decode(s, static_cast<const unsigned long long *>(e->sp_comp_a.p), P, L.t0, nk, nt);
  } else {             // the dense grid compacted as tad_aggregate does
    launch_count_flags(s, g, true, bk.kcnt);
    launch_scan(s, bk.kcnt, bk.koff, g.K, static_cast<unsigned long long *>(e->scan_scratch.p));
    launch_emit_points(s, g, L, bk.koff, nk, nt, static_cast<unsigned long long *>(e->hs_val.p));
    *poff = bk.koff;
    *nv = static_cast<const unsigned long long *>(e->hs_val.p);
  }
}

static int ensure_hist_verdicts(JobCtx *e, uint64_t P_cap) {   // per point: noise u8 | cnt u32 | row u64 (+ 1)
  const uint64_t pc = P_cap ? P_cap : 1;
  int rc;
  if ((rc = ensure(e, e->hs_noise, pc)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_cnt, pc * 4)) != TAD_OK) return rc;
  return ensure(e, e->hs_row, (pc + 1) * 8);
}

// DBSCAN's verdicts of the points hb names (nk, nv, P_dev, P_cap) against the history (hoff, hval), and their rows: the row total lands in
// the job's tail.  The scan's scratch is the caller's (e->scan_scratch, sized for P_cap).  No point, no launch: hb keeps no verdicts.
int hist_verdicts(JobCtx *e, const unsigned long long *hoff, const unsigned long long *hval, const JobParams &jp, HistBatch *hb) {
  int rc;
  if ((rc = ensure_hist_verdicts(e, hb->P_cap)) != TAD_OK) return rc;
  if (hb->P_cap == 0) return TAD_OK;
  uint8_t *noise = static_cast<uint8_t *>(e->hs_noise.p);
  uint32_t *cnt = static_cast<uint32_t *>(e->hs_cnt.p);
  unsigned long long *row = static_cast<unsigned long long *>(e->hs_row.p);
  launch_hist_verdict(e->stream, hb->nk, hb->nv, hb->P_dev, hb->P_cap, hoff, hval, jp.eps, jp.min_samples, jp.all_points, noise, cnt);
  launch_scan(e->stream, cnt, row, hb->P_cap, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
  hb->noise = noise; hb->cnt = cnt; hb->row = row;
  return TAD_OK;
}

// The rows of a batch of points that DBSCAN, ARIMA or DROP judged (hist_verdicts, stream_arima_batch, state_drop_batch); mom: the moments
// DBSCAN's stddev column comes from.  EWMA's emits are its callers' own.
void emit_point_rows(hipStream_t s, const JobParams &jp, const HistBatch &hb, const ArimaBatch &ab, const DropBatch &db, const StreamState &mom,
                     OutRows out) {
  if (jp.algo == TAD_ALGO_ARIMA)
    launch_as_emit(s, ab.P, hb.nk, hb.nt, hb.nv, ab.tidx, ab.sigma, ab.pcalc, ab.pflag, ab.rows, ab.row_off, jp.all_points, out);
  else if (jp.algo == TAD_ALGO_DBSCAN)
    launch_hist_emit(s, hb.nk, hb.nt, hb.nv, hb.P_dev, hb.P_cap, hb.noise, hb.cnt, hb.row, mom, jp.all_points, out);
  else if (jp.algo == TAD_ALGO_DROP)
    launch_ds_emit(s, hb.nk, hb.nt, hb.nv, hb.P_dev, hb.P_cap, db.flag, db.cnt, db.row, db.keys, jp.all_points, out);
}

// A batch's points (key k's nt / nv at [poff[k], poff[k + 1]), at most P_cap) appended to what every key holds, current copies into
// candidate copies: 2. a history state sorts every key's new values and 3. merges them with its history (tad_history.hip); 3'. a series
// state appends them to its series, 3''. and their times beside them (the same offsets, written again).  long_list / long_count and
// chunks / coff: the per-key scratch of the sort and of the merge, in the caller's block.
static void append_batch(JobCtx *e, tad_state *st, const unsigned long long *poff, const long long *nt, const unsigned long long *nv, uint64_t P_cap,
                         uint32_t *long_list, unsigned int *long_count, uint32_t *chunks, unsigned long long *coff) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const int cur = st->cur, cand = cur ^ 1;
  if (st->history) {
    unsigned long long *ns = static_cast<unsigned long long *>(e->hs_sorted.p);
    launch_hist_sort(s, nv, poff, K, ns, long_list, long_count);
    launch_hist_merge(s, K, st->hist.off[cur], st->hist.val.p[cur], poff, ns, st->hist.off[cand], st->hist.val.p[cand], chunks, coff,
                      static_cast<unsigned long long *>(e->scan_scratch.p), hist_merge_chunks_bound(K, st->hist.len[cur] + P_cap));
  }
  if (st->series)
    launch_series_append(s, K, st->ser.off[cur], st->ser.val.p[cur], poff, nv, st->ser.off[cand], st->ser.val.p[cand]);
  if (st->times)
    launch_series_append(s, K, st->ser.off[cur], reinterpret_cast<const unsigned long long *>(st->ser_times.p[cur]), poff,
                         reinterpret_cast<const unsigned long long *>(nt), st->ser.off[cand], reinterpret_cast<unsigned long long *>(st->ser_times.p[cand]));
}

// One batch on a history and / or series state (tad.h, TAD_STATE_HISTORY / TAD_STATE_SERIES), after the stream count pass and before the
// job's tail is read: the batch's new points in (key, time) order; a history state sorts them per key and merges them with the current
// history into the candidate arena (tad_history.hip); a series state appends them to every key's series in the candidate arena; a DBSCAN
// batch also judges the new points against the merged history and scans their rows into the row total.  Writes only candidate memory:
// history and series become current with the moments, when the batch succeeds.  sparse_poff: a sparse batch's point offsets (P points in
// e->sp_comp_a / e->sp_val_a); otherwise the dense grid g is compacted, at most P_bound points.
int stream_history_batch(JobCtx *e, tad_state *st, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, uint64_t P_bound,
                         const JobParams &jp, HistBatch *hb) {
  hipStream_t s = e->stream;
  const uint64_t K = g.K;
  const int cur = st->cur, cand = cur ^ 1;
  const bool dbscan = jp.algo == TAD_ALGO_DBSCAN;
  const uint64_t P_cap = sparse_poff ? P : P_bound;
  BatchKeys bk;
  int rc;
  // the candidate arenas first: an allocation failure leaves the state, its history and its series as they are
  if ((rc = state_grow_candidates(e, st, P_cap)) != TAD_OK) return rc;
  if ((rc = ensure_batch_points(e, K, P_cap, sparse_poff != nullptr, &bk)) != TAD_OK) return rc;
  if (dbscan && (rc = ensure_hist_verdicts(e, P_cap)) != TAD_OK) return rc;   // (before the first launch: hist_verdicts then allocates nothing)
  unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
  long long *nt = static_cast<long long *>(e->hs_t.p);
  const unsigned long long *poff, *nv;
  batch_points(e, bk, g, L, sparse_poff, P, &poff, &nv);   // 1.
  append_batch(e, st, poff, nt, nv, P_cap, bk.kcnt, bk.long_count, bk.kcnt, bk.coff);   // 2. to 3''. (the sort's long list, then the merge's chunk counts, in kcnt)
  HIP_TRY(e, hipMemcpyAsync(static_cast<unsigned char *>(e->counters.p) + kTailHistLen, poff + K, 8, hipMemcpyDeviceToDevice, s));
  hb->nk = nk; hb->nt = nt; hb->nv = nv; hb->poff = poff; hb->P_dev = poff + K; hb->P_cap = P_cap;
  // 4. verdicts of the new points against the merged history; 5. their rows
  return dbscan ? hist_verdicts(e, st->hist.off[cand], st->hist.val.p[cand], jp, hb) : TAD_OK;
}

// the candidate copy of a series state's series and times, as a merge writes it
static MergeInto candidate_series(const tad_state *st) {
  const int cand = st->cur ^ 1;
  MergeInto m;
  m.soff = st->ser.off[cand]; m.sval = st->ser.val.p[cand]; m.st = st->ser_times.p[cand];
  return m;
}

// tad_state_merge_changes / tad_state_replace_changes: where the report of this attempt is written.  The counters, and the per-key array
// when the caller's is in host memory (or absent: the changed keys are counted from it), live in context workspace; a device array of
// the caller's is written in place (on a failure its content is unspecified).
int merge_report_begin(JobCtx *e, const tad_state *st, MergeCall *mc) {
  const tad_changes *ch = mc->ch;
  int rc;
  mc->report_staged = ch->key_since == nullptr || ch->memory == TAD_MEM_HOST;
  if ((rc = carve_buf(e, e->mg_report, &mc->report, merge_report_layout, st->K, mc->report_staged)) != TAD_OK) return rc;
  if (!mc->report_staged) mc->report.since = reinterpret_cast<long long *>(ch->key_since);
  mc->counted = ChangeCounters{};
  launch_merge_report_fill(e->stream, st->K, mc->report);
  return TAD_OK;
}

// One tad_state_merge or tad_state_replace batch (tad.h; kernels in tad_merge.hip), in the place of a stream batch's count pass: the batch's
// points in (key, time) order are classified against the current series, then either appended as a stream batch appends them (nothing
// inserted, combined, too old or erased) or merged by time into the candidate series, times, history and moments.  A point at a time its
// key holds is combined with the held value (op_max: the maximum, else the sum) or, mc->replace, takes its place; with mc->ranged every
// old point of every key inside [from_t, to_t) that the batch does not name is erased — by a batch without a live row (g.K == 0) or
// without points too.  Writes candidate memory and context workspace only; mc->changed tells run_job_locked whether the candidates are to
// become current.  One host round trip for the Stage-0 error word and the classification's counters — a Stage-0 error leaves the rest
// undone (run_job_locked retries or reports it) — and, ranged, a second one for the erased total: the append path and the arena sizes hang
// on it, and it is read before anything is written.
int state_merge_batch(JobCtx *e, tad_state *st, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, uint64_t P_bound, bool op_max,
                      double alpha, MergeCall *mc) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;   // (== g.K, the batch's keys, unless the batch has no live row)
  const int cur = st->cur, cand = cur ^ 1;
  const bool no_batch = g.K == 0;
  const uint64_t P_cap = no_batch ? 0 : (sparse_poff ? P : P_bound);
  const uint64_t pc = P_cap ? P_cap : 1;
  const uint64_t S = st->ser.len[cur], H = st->hist.len[cur];
  BatchKeys bk;
  MergePts mp;
  MergeKeys mk;
  ReplaceKeys rk{};
  int rc;
  mc->changed = false;
  mc->added = mc->erased = mc->emptied = 0;
  // the candidate arenas first: an allocation failure leaves the state as it is
  if ((rc = state_grow_candidates(e, st, P_cap)) != TAD_OK) return rc;
  if ((rc = ensure_batch_points(e, K, P_cap, sparse_poff != nullptr, &bk)) != TAD_OK) return rc;
  if ((rc = carve_buf(e, e->mg_pts, &mp, merge_pts_layout, pc)) != TAD_OK) return rc;
  if ((rc = carve_buf(e, e->mg_keys, &mk, merge_keys_layout, K)) != TAD_OK) return rc;
  MergeCounters *mcnt = mk.mcnt;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  HistBatch hb;
  hb.nk = static_cast<const unsigned long long *>(e->hs_key.p);
  hb.nt = static_cast<const long long *>(e->hs_t.p);
  if (mc->replace) {   // the erased runs and their scan are all zero until the range kernel says otherwise; pzero stays zero
    if ((rc = carve_buf(e, e->rp_keys, &rk, replace_keys_layout, K)) != TAD_OK) return rc;
    HIP_TRY(e, hipMemsetAsync(e->rp_keys.p, 0, carved_bytes(replace_keys_layout, K), s));
    hb.poff = rk.pzero;
  }
  if (!no_batch) batch_points(e, bk, g, L, sparse_poff, P, &hb.poff, &hb.nv);
  hb.P_dev = hb.poff + K;
  hb.P_cap = P_cap;
  const StateView old = series_view(st, cur);
  MergeInto into = candidate_series(st);
  MergeRule how;
  how.replace = mc->replace; how.op_max = op_max;
  if (mc->ranged) { how.range = &rk; how.from = (long long)mc->from_t; how.to = (long long)mc->to_t; }
  if (mc->ch) how.report = &mc->report;   // (merge_report_begin filled it for this attempt)
  // 1. classify; the first round trip: Stage 0's error word, the point count, the classification's counters
  HIP_TRY(e, hipMemsetAsync(mcnt, 0, sizeof(MergeCounters), s));
  launch_merge_classify(s, hb, old, (long long)mc->keep_from, mp, mcnt);
  unsigned char *hm = e->tail_host + kTailMoments;   // (the moment partials' place in the pinned tail: a merge has none)
  HIP_TRY(e, hipMemcpyAsync(e->ctr_host, e->counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(hm, mcnt, sizeof(MergeCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(hm + sizeof(MergeCounters), hb.P_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (e->ctr_host->err != 0) return TAD_OK;
  MergeCounters c;
  unsigned long long points = 0, erased = 0;
  memcpy(&c, hm, sizeof c);
  memcpy(&points, hm + sizeof c, 8);
  tad_merge_stats &ms = mc->stats;
  ms.batch_points = points;
  ms.points_too_old = c.too_old;
  ms.points_appended = c.appended;
  ms.points_inserted = c.inserted;
  ms.points_combined = c.combined;
  ms.keys_touched = ms.keys_replayed = 0;
  // 2. a replace scans its replaced points here (the poff the points came with is sound: Stage 0 raised no error): the erased runs of a
  //    range on a state that holds points count them; then the runs' scan and the second round trip: the erased total
  if (mc->replace) launch_scan(s, mp.f_hit, mp.roff, P_cap, scratch);
  if (mc->ranged && S != 0) {
    launch_merge_range(s, hb, old, mp, how);
    launch_scan(s, rk.ecnt, rk.eoff, K, scratch);
    HIP_TRY(e, hipMemcpyAsync(hm, rk.eoff + K, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    memcpy(&erased, hm, 8);
  }
  if (c.appended + c.inserted + c.combined + erased == 0) return TAD_OK;   // nothing to place, nothing to erase: the state stays as it is
  const uint64_t added = c.inserted + c.appended;
  // every point is newer than what its key held and nothing leaves: the append path of a stream batch, the moments continued from the
  // stored state (no key replays)
  const bool append = c.inserted == 0 && c.combined == 0 && c.too_old == 0 && erased == 0;
  if (append) {
    append_batch(e, st, hb.poff, hb.nt, hb.nv, P_cap, mk.long_list, mk.long_count, mk.chunks_h, mk.coff_h);
    if (how.report) launch_merge_report_keys(s, K, hb.poff, hb.nt, *how.report);   // a key's changed points: its batch segment
  } else {
    const uint64_t lost = c.combined + erased;   // values that leave the history
    unsigned long long *hrem_s = mp.hrem_s;
    if (erased) {   // (a state that shrinks may give arenas back: the candidate copies anew)
      if ((rc = state_size_arenas(e, st, cand, S + added - erased, st->history ? H + added - erased : 0, true, "tad_state_replace")) != TAD_OK) return rc;
      into = candidate_series(st);
    }
    if (st->history) {
      into.hrem = mp.hrem;
      if (lost && (rc = ensure(e, e->mg_hist, (H ? H : 1) * 8)) != TAD_OK) return rc;
      if (lost && mc->replace) {   // (a replace's losses may outnumber the batch's points: a block of their own)
        ReplaceLoss rl;
        if ((rc = carve_buf(e, e->rp_loss, &rl, replace_loss_layout, lost)) != TAD_OK) return rc;
        into.hrem = rl.hrem;
        hrem_s = rl.hrem_s;
      }
    }
    // 3. the remaining scans; per key: candidate offsets, the history's packed gains / losses, chunk counts, who replays, who is emptied
    launch_scan(s, mp.f_nh, mp.nhoff, P_cap, scratch);
    launch_scan(s, mp.f_kept, mp.aoff, P_cap, scratch);
    if (!mc->replace) launch_scan(s, mp.f_hit, mp.roff, P_cap, scratch);
    launch_merge_keys(s, hb, old, into, mp, mk, how);
    launch_scan(s, mk.chunks_s, mk.coff_s, K, scratch);
    // 4. series and times merged by time (and the history's gains and losses packed)
    launch_merge_series(s, hb, old, into, mp, mk, how);
    if (how.report) launch_merge_report_keys(s, K, nullptr, nullptr, *how.report);
    if (st->history) {   // 5. the combined and erased values leave the history (through the scratch arena), then the batch's values enter
      const unsigned long long *hoff_from = st->hist.off[cur], *hval_from = st->hist.val.p[cur];
      if (lost) {
        unsigned long long *hmid = static_cast<unsigned long long *>(e->mg_hist.p);
        launch_hist_sort(s, into.hrem, mk.rkoff, K, hrem_s, mk.long_list, mk.long_count);
        launch_scan(s, mk.chunks_h, mk.coff_h, K, scratch);
        // (mk.chunks_h gives an empty key no chunk: not the one-chunk-at-least counts of a trim)
        launch_hist_subtract(s, trim_chunks_bound(K, H), mk.coff_h, K, st->hist.off[cur], st->hist.val.p[cur], mk.rkoff, hrem_s, mk.hoff_mid, hmid, false);
        hoff_from = mk.hoff_mid;
        hval_from = hmid;
      }
      launch_hist_sort(s, mp.hadd, mk.akoff, K, mp.hadd_s, mk.long_list, mk.long_count);
      launch_hist_merge(s, K, hoff_from, hval_from, mk.akoff, mp.hadd_s, st->hist.off[cand], st->hist.val.p[cand], mk.chunks_h, mk.coff_h, scratch,
                        hist_merge_chunks_bound(K, H + P_cap));
    }
  }
  // 6. the moments
  launch_merge_moments(s, old, into, append ? nullptr : mk.replay, alpha, state_view(st, cand), mcnt);
  HIP_TRY(e, hipMemcpyAsync(hm, mcnt, sizeof(MergeCounters), hipMemcpyDeviceToHost, s));
  if (how.report) HIP_TRY(e, hipMemcpyAsync(hm + sizeof(MergeCounters), how.report->cc, sizeof(ChangeCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  memcpy(&c, hm, sizeof c);
  if (how.report) {
    memcpy(&mc->counted, hm + sizeof c, sizeof mc->counted);
    if (append) mc->counted.points = c.appended;   // (the series kernel, which counts them, did not run)
  }
  ms.keys_touched = c.keys_touched;
  ms.keys_replayed = c.keys_replayed;
  mc->changed = true;
  mc->added = added;
  mc->erased = erased;
  mc->emptied = c.keys_emptied;
  return TAD_OK;
}

constexpr uint64_t kStreamFitWaves = 4096;   // k_arima_fit_list: wavefronts a batch aims for (two per SIMD twice over)

// One ARIMA batch on a series state (tad.h, TAD_STATE_SERIES), after stream_history_batch appended the new points to the candidate series:
// the touched keys' Box-Cox fits over their whole series, the fits of the new points only, verdicts and the row count (tad_arima.hip).
// Writes only workspace memory.  A batch whose Stage 0 or stream pass raised an error (a late row) runs no fit: the caller fails it.
// v: the series and moments to read — the state's candidate copy for a batch; the current one, or a window's view, for tad_run_state /
// tad_run_state_window, whose HistBatch names every series point as new (poff = the series offsets).
int stream_arima_batch(JobCtx *e, const StateView &v, const HistBatch &hb, const JobParams &jp, DevCounters *ctr, ArimaBatch *ab) {
  hipStream_t s = e->stream;
  const uint64_t K = v.K;
  const unsigned long long *soff = v.soff, *sval = v.sval;
  int rc;
  ArimaKeys ak;
  if ((rc = carve_buf(e, e->as_key, &ak, arima_keys_layout, K)) != TAD_OK) return rc;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  launch_as_touch(s, K, soff, hb.poff, ak.touched, ak.len8, ak.tmax);
  launch_scan(s, ak.touched, ak.tidx, K, scratch);
  launch_scan(s, ak.len8, ak.yoffk, K, scratch);
  unsigned long long hv[3] = {0, 0, 0};   // new points, slots, packed doubles
  unsigned int tmax = 0;
  HIP_TRY(e, hipMemcpyAsync(&hv[0], hb.P_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&hv[1], ak.tidx + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&hv[2], ak.yoffk + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&tmax, ak.tmax, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(e->ctr_host, ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  const uint64_t P = hv[0], Kt = hv[1], S8 = hv[2];
  ab->P = 0;
  if (e->ctr_host->err != 0 || P == 0) return TAD_OK;   // (the caller reads the error from the tail)
  // per new point, and the packed series with its slack
  ArimaPts ap;
  ArimaSeries as;
  if ((rc = carve_buf(e, e->as_pt, &ap, arima_pts_layout, P)) != TAD_OK) return rc;
  if ((rc = carve_buf(e, e->as_ser, &as, arima_series_layout, S8, tmax)) != TAD_OK) return rc;
  HIP_TRY(e, hipMemsetAsync(ap.pflag, 0, P, s));
  HIP_TRY(e, hipMemsetAsync(as.ysk, 0, as.ser * 8, s));   // (the slack: finite values for idle lanes)
  launch_as_prep(s, K, soff, sval, hb.poff, v.mom, ak.tidx, ak.yoffk, as.lx, as.ysk, ak.sl, ap.pcalc, ap.pflag, ctr);
  // the fits: counted per position, listed, their wavefronts laid out on the host (heaviest position first)
  const uint64_t npos = (uint64_t)tmax + 1;
  ArimaPos pos;
  if ((rc = carve_buf(e, e->as_pos, &pos, arima_pos_layout, npos)) != TAD_OK) return rc;
  HIP_TRY(e, hipMemsetAsync(pos.pcnt, 0, npos * 4, s));
  launch_as_list(s, Kt, ak.sl, false, pos.pcnt, nullptr, nullptr, nullptr);
  std::vector<uint32_t> hcnt;
  std::vector<unsigned long long> hoff;
  std::vector<uint32_t> wave_pos;
  try { hcnt.resize(npos); hoff.resize(npos + 1); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  HIP_TRY(e, hipMemcpyAsync(hcnt.data(), pos.pcnt, npos * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  uint64_t nfits = 0;
  for (uint64_t p = 0; p < npos; ++p) { hoff[p] = nfits; nfits += hcnt[p]; }
  hoff[npos] = nfits;
  const uint64_t chunk = nfits / kStreamFitWaves < 64 ? 64 : (nfits / kStreamFitWaves + 63) / 64 * 64;   // fits per wavefront and position
  try {
    for (uint64_t p = npos; p-- > 0;)
      for (uint64_t w = 0; w < (hcnt[p] + chunk - 1) / chunk; ++w) wave_pos.push_back((uint32_t)p);
  } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  const uint64_t waves = wave_pos.size();
  ArimaFits fits;
  if ((rc = carve_buf(e, e->as_fit, &fits, arima_fits_layout, nfits, waves)) != TAD_OK) return rc;
  if (nfits) {
    HIP_TRY(e, hipMemcpyAsync(pos.loff, hoff.data(), (npos + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemcpyAsync(fits.wpos, wave_pos.data(), waves * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemsetAsync(pos.pcnt, 0, npos * 4, s));
    launch_as_list(s, Kt, ak.sl, true, pos.pcnt, pos.loff, fits.list, fits.fpos);
    const size_t wsb = arima_stream_ws_bytes(nfits, npos, waves);
    if ((rc = ensure(e, e->as_ws, wsb)) != TAD_OK) return rc;
    const FitListArgs fa{fits.wpos, pos.pcnt, pos.loff, fits.list, hb.nv, ap.pcalc, ap.pflag};
    // the fit yields to whole-CU jobs of other contexts like tad_run's (arima_yield_loop); this job's own claim is dropped meanwhile
    const bool held = e->hold && e->hold->held;
    if (held) e->hold->release();
    const unsigned int *yielded_dev = nullptr;
    if (launch_arima_stream_fit(s, true, nfits, npos, waves, fits.fpos, as.ysk, ak.sl, fa, jp.maxiter, ctr, e->as_ws.p, e->eng->pause_dev, &yielded_dev, 0) != 0)
      return fail(e, TAD_ERR_HIP, "ARIMA launch failed");
    if ((rc = arima_yield_loop(e, yielded_dev, [&](uint32_t grace, const unsigned int **yd) {
           return launch_arima_stream_fit(s, false, nfits, npos, waves, fits.fpos, as.ysk, ak.sl, fa, jp.maxiter, ctr, e->as_ws.p, e->eng->pause_dev, yd, grace);
         })) != TAD_OK)
      return rc;
    if (held) e->hold->acquire();
  }
  // rows of the new points (the row total lands in the job's tail)
  launch_as_rows(s, P, hb.nk, ak.tidx, ak.sl.ok, ap.pflag, jp.all_points, ap.rows);
  launch_scan(s, ap.rows, ap.row_off, P, scratch, dev_total(e));
  ab->P = P; ab->tidx = ak.tidx; ab->sigma = ak.sl.sigma; ab->pcalc = ap.pcalc; ab->pflag = ap.pflag; ab->rows = ap.rows; ab->row_off = ap.row_off;
  return TAD_OK;
}

// The drop detector over a state's series (tad.h: tad_drop_state / tad_drop_stream; kernels: tad_drop_state.hip): per-key mean / std over
// the WHOLE series of v, the verdicts of the points hb names and their rows (the row total lands in the job's tail).  touched_only (a
// stream batch: v is the candidate series, hb the batch's new points): only keys with new points are routed, read and judged.  Otherwise
// (tad_drop_state: hb names every series point, poff = the series offsets) list / lcount are the routing launch_win_route left, and the
// job's moments partials are merged from the per-key pairwise mean and m2.  Writes context workspace only, per key and per judged point.
int state_drop_batch(JobCtx *e, const StateView &v, const HistBatch &hb, const JobParams &jp, bool touched_only, unsigned long long coop_min,
                     uint32_t *list, unsigned int *lcount, DevCounters *ctr, DropBatch *db) {
  hipStream_t s = e->stream;
  const uint64_t K = v.K, pc = hb.P_cap ? hb.P_cap : 1;
  int rc;
  DropStateKeys dk;
  DropPts dp;
  if ((rc = carve_buf(e, e->ds_key, &dk, drop_state_keys_layout, K)) != TAD_OK) return rc;
  if ((rc = carve_buf(e, e->ds_pt, &dp, drop_pts_layout, pc)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > pc ? K : pc) * sizeof(unsigned long long))) != TAD_OK) return rc;
  if (touched_only) launch_ds_route(s, K, v.soff, hb.poff, coop_min, list, lcount);
  launch_ds_stats(s, K, v.soff, v.sval, touched_only ? hb.poff : nullptr, coop_min, list, lcount, jp.drop_min_samples, dk, ctr);
  if (!touched_only) launch_moments(s, K, dk.n, dk.mean, dk.m2, dev_moments(e), ctr);   // (and n_keys / n_points)
  if (hb.P_cap) {
    launch_ds_verdict(s, hb.nk, hb.nv, hb.P_dev, hb.P_cap, dk, jp.drop_nsigma, jp.all_points, dp.flag, dp.cnt);
    launch_scan(s, dp.cnt, dp.row, hb.P_cap, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
  }
  db->keys = dk; db->flag = dp.flag; db->cnt = dp.cnt; db->row = dp.row;
  return TAD_OK;
}

}  // namespace tadh

extern "C" {

// tad.h: the periodical drop job, one batch.  The batch runs as a stream batch of the EWMA kind does (run_job_locked: Stage 0, the count
// pass into the candidate state, stream_history_batch), then state_drop_batch judges the new points; tad_run_stream itself keeps
// refusing TAD_ALGO_DROP.
int tad_drop_stream(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out) {
  const char *who = "tad_drop_stream";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !cols || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job, cols and out must not be NULL", who);
  *out = nullptr;
  if (job->algo != TAD_ALGO_DROP)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be DROP (tad_run_stream streams EWMA, DBSCAN and ARIMA)", who);
  if (!st->series)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series (tad_state_create_ex with TAD_STATE_SERIES); state unchanged", who);
  if (cols->num_keys != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: batch declares %llu keys, the state holds %llu (they must be equal)", who,
                (unsigned long long)cols->num_keys, (unsigned long long)st->K);
  {
    const int vrc = validate_job_columns(eng, job, cols, who);
    if (vrc != TAD_OK) return vrc;
  }
  if (!(job->ewma_alpha >= 0.0 && job->ewma_alpha <= 1.0) || !(job->drop_nsigma >= 0.0) || job->drop_min_samples < 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: detector parameter out of range", who);
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times); state unchanged", who);
  int rc = call.enter(who, job->id);
  if (rc != TAD_OK) return rc;
  PauseHold hold(eng);     // (declared after the call's context: dropped before the context goes back to the pool)
  call.e->hold = &hold;
  return run_job_locked(call.e, job, cols, out_memory, out, nullptr, st, 0);
}

// what tad_state_merge and tad_state_replace refuse alike (who: the call's name), then the batch run as a stream batch does up to the end
// of Stage 0 (run_job_locked with the context's merge mode set) and state_merge_batch in the count pass's place
static int run_merge_call(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, const char *who, MergeCall *mc) {
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES): "
                                               "without them it does not know where a late point belongs; state unchanged", who);
  if (job->flags & TAD_FLAG_EMIT_ALL_POINTS)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_EMIT_ALL_POINTS asks for rows; a merge emits none (tad_run_state judges the window)", who);
  if (!(job->ewma_alpha >= 0.0 && job->ewma_alpha <= 1.0)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: ewma_alpha out of range", who);
  if (cols->num_keys != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: batch declares %llu keys, the state holds %llu (they must be equal)", who,
                (unsigned long long)cols->num_keys, (unsigned long long)st->K);
  {
    const int vrc = validate_job_columns(eng, job, cols, who);
    if (vrc != TAD_OK) return vrc;
  }
  tad_job j = *job;   // the detector is not run: a stream batch of the EWMA kind up to the end of Stage 0
  j.algo = TAD_ALGO_EWMA;
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times); state unchanged", who);
  int rc = call.enter(who, j.id);
  if (rc != TAD_OK) return rc;
  PauseHold hold(eng);     // (declared after the call's context: dropped before the context goes back to the pool)
  call.e->hold = &hold;
  call.e->merge = mc;
  tad_result *none = nullptr;
  rc = run_job_locked(call.e, &j, cols, TAD_MEM_DEVICE, &none, nullptr, st, 0);
  call.e->merge = nullptr;
  return rc;
}

// what a call with a report refuses about it, before anything runs (the state's num_keys does not change under a call's feet: only
// tad_state_grow / tad_state_compact change it, and the caller orders those)
static int check_changes(tad_engine *eng, const tad_state *st, tad_changes *ch, const char *who) {
  ch->keys_changed = ch->points_changed = 0;
  ch->min_t = ch->max_t = 0;
  if (ch->memory != TAD_MEM_HOST && ch->memory != TAD_MEM_DEVICE)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the report's memory must be TAD_MEM_HOST or TAD_MEM_DEVICE; state unchanged", who);
  if (!ch->key_since && ch->len != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the report's key_since is NULL with len %llu (NULL goes with len 0: counters only); state unchanged", who,
                (unsigned long long)ch->len);
  if (ch->key_since && ch->len != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the report's len is %llu, the state holds %llu keys (they must be equal); state unchanged", who,
                (unsigned long long)ch->len, (unsigned long long)st->K);
  if (reinterpret_cast<uintptr_t>(ch->key_since) % 8 != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the report's key_since must be 8-byte aligned; state unchanged", who);
  return TAD_OK;
}

// after a successful call: the counters (0, 0 for min_t / max_t without a changed point)
static void report_counters(const MergeCall &mc, tad_changes *ch) {
  ch->keys_changed = mc.counted.keys;
  ch->points_changed = mc.counted.points;
  if (mc.counted.points != 0) { ch->min_t = mc.counted.min_t; ch->max_t = mc.counted.max_t; }
}

// tad.h: a batch placed by time.
int tad_state_merge_changes(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, int64_t keep_from_t, tad_merge_stats *stats,
                            tad_changes *ch) {
  const char *who = ch ? "tad_state_merge_changes" : "tad_state_merge";
  if (stats) memset(stats, 0, sizeof *stats);
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !cols) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and cols must not be NULL", who);
  if (ch) {
    const int crc = check_changes(eng, st, ch, who);
    if (crc != TAD_OK) return crc;
  }
  MergeCall mc;
  mc.keep_from = keep_from_t;
  mc.ch = ch;
  const int rc = run_merge_call(eng, st, job, cols, who, &mc);
  if (rc == TAD_OK && stats) *stats = mc.stats;
  if (rc == TAD_OK && ch) report_counters(mc, ch);
  return rc;
}

int tad_state_merge(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, int64_t keep_from_t, tad_merge_stats *stats) {
  return tad_state_merge_changes(eng, st, job, cols, keep_from_t, stats, nullptr);
}

// tad.h: a batch that replaces what the state holds, with TAD_REPLACE_RANGE everything the state holds inside [from_t, to_t).
int tad_state_replace_changes(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, uint32_t flags, int64_t from_t,
                              int64_t to_t, int64_t keep_from_t, tad_replace_stats *stats, tad_changes *ch) {
  const char *who = ch ? "tad_state_replace_changes" : "tad_state_replace";
  if (stats) memset(stats, 0, sizeof *stats);
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !cols) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and cols must not be NULL", who);
  if (ch) {
    const int crc = check_changes(eng, st, ch, who);
    if (crc != TAD_OK) return crc;
  }
  if (flags & ~TAD_REPLACE_RANGE) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", who, flags & ~TAD_REPLACE_RANGE);
  const bool ranged = (flags & TAD_REPLACE_RANGE) != 0;
  if (!ranged && (from_t != 0 || to_t != 0))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: from_t / to_t need TAD_REPLACE_RANGE (without it nothing is erased); state unchanged", who);
  if (from_t != 0 && to_t != 0 && from_t > to_t)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: from_t %lld is after to_t %lld; state unchanged", who, (long long)from_t, (long long)to_t);
  MergeCall mc;
  mc.ch = ch;
  mc.keep_from = keep_from_t;
  mc.replace = true;
  mc.ranged = ranged && !(from_t != 0 && from_t == to_t);   // (from_t == to_t non-zero: an empty range)
  mc.from_t = from_t;
  mc.to_t = to_t;
  const int rc = run_merge_call(eng, st, job, cols, who, &mc);
  if (rc == TAD_OK && ch) report_counters(mc, ch);
  if (rc == TAD_OK && stats) {
    const tad_merge_stats &m = mc.stats;
    stats->rows_in = m.rows_in; stats->rows_used = m.rows_used; stats->batch_points = m.batch_points;
    stats->points_too_old = m.points_too_old; stats->points_appended = m.points_appended; stats->points_inserted = m.points_inserted;
    stats->points_replaced = m.points_combined; stats->points_erased = mc.erased; stats->keys_emptied = mc.emptied;
    stats->keys_touched = m.keys_touched; stats->keys_replayed = m.keys_replayed;
    stats->stage0_path = m.stage0_path; stats->stage0_attempts = m.stage0_attempts; stats->job_context = m.job_context;
    stats->ms_stage0 = m.ms_stage0; stats->ms_replace = m.ms_merge; stats->ms_total = m.ms_total;
  }
  return rc;
}

int tad_state_replace(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, uint32_t flags, int64_t from_t, int64_t to_t,
                      int64_t keep_from_t, tad_replace_stats *stats) {
  return tad_state_replace_changes(eng, st, job, cols, flags, from_t, to_t, keep_from_t, stats, nullptr);
}

}  // extern "C"