// tad_capi.cpp — what the entry points of include/tad.h share (key buffers, the rows result and its epilogue, the moments' merge), the batches
// on a streaming state that the job's count pass runs (history, series, merge, ARIMA, DROP), and the state calls: tad_run_state,
// tad_run_state_window, tad_drop_state, their *_keys forms, tad_drop_stream, tad_state_merge.  The batch job itself (run_job_locked: lattice, Stage 0, count,
// retries) is tad_capi_job.cpp; the life of a tad_state is tad_capi_state.cpp.
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
  const size_t bytes = result_bytes(rows, with_anomaly);
  int rc = alloc_device_block(e, bytes, dev_block);
  if (rc != TAD_OK) { delete rp; return rc; }
  carve(dev_block->base, rows, with_anomaly, dev_rows);
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
  const size_t bytes = result_bytes(rows, with_anomaly);
  void *h = malloc(bytes);
  if (!h) { release_block(e, dev_block.base, dev_block.cap); return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory for %zu result bytes", bytes); }
  hipError_t r = hipMemcpyAsync(h, dev_block.base, bytes, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  release_block(e, dev_block.base, dev_block.cap);
  if (r != hipSuccess) { free(h); return fail(e, TAD_ERR_HIP, "result copy failed: %s", hipGetErrorString(r)); }
  OutRows ho;
  carve(h, rows, with_anomaly, &ho);
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
// and per-key offsets in *nv / *poff.  ensure_batch_points sizes the buffers both share (hs_key, hs_t, hs_sorted, hs_koff: dense point
// offsets | chunk offsets, K + 1 each; hs_kcnt: per-key counts / long-sort list / chunks | long-list length; the scan scratch).
static int ensure_batch_points(JobCtx *e, uint64_t K, uint64_t P_cap, bool sparse) {
  const size_t kpad = (size_t)((K + 3) & ~3ull);
  const uint64_t pc = P_cap ? P_cap : 1;
  int rc;
  if ((rc = ensure(e, e->hs_key, pc * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_t, pc * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_sorted, pc * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_koff, (kpad + 4) * 16)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->hs_kcnt, kpad * 4 + 64)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > pc ? K : pc) * sizeof(unsigned long long))) != TAD_OK) return rc;
  if (!sparse && (rc = ensure(e, e->hs_val, pc * 8)) != TAD_OK) return rc;
  return TAD_OK;
}

static void batch_points(JobCtx *e, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, const unsigned long long **poff,
                  const unsigned long long **nv) {
  hipStream_t s = e->stream;
  unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
  long long *nt = static_cast<long long *>(e->hs_t.p);
  if (sparse_poff) {   // the sorted unique points of the sparse Stage 0
    *poff = sparse_poff;
    *nv = static_cast<const unsigned long long *>(e->sp_val_a.p);
    launch_hist_decode(s, static_cast<const unsigned long long *>(e->sp_comp_a.p), P, L.t0, nk, nt);
  } else {             // the dense grid compacted as tad_aggregate does
    unsigned long long *koff = static_cast<unsigned long long *>(e->hs_koff.p);
    uint32_t *kcnt = static_cast<uint32_t *>(e->hs_kcnt.p);
    launch_count_flags(s, g, true, kcnt);
    launch_scan(s, kcnt, koff, g.K, static_cast<unsigned long long *>(e->scan_scratch.p));
    launch_emit_points(s, g, L, koff, nk, nt, static_cast<unsigned long long *>(e->hs_val.p));
    *poff = koff;
    *nv = static_cast<const unsigned long long *>(e->hs_val.p);
  }
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
  const size_t kpad = (size_t)((K + 3) & ~3ull);
  int rc;
  // the candidate arenas first: an allocation failure leaves the state, its history and its series as they are
  const uint64_t need = st->hist.len[cur] + P_cap;
  if ((rc = state_grow_candidates(e, st, P_cap)) != TAD_OK) return rc;
  const uint64_t pc = P_cap ? P_cap : 1;
  if ((rc = ensure_batch_points(e, K, P_cap, sparse_poff != nullptr)) != TAD_OK) return rc;
  if (dbscan) {
    if ((rc = ensure(e, e->hs_noise, pc)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->hs_cnt, pc * 4)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->hs_row, (pc + 1) * 8)) != TAD_OK) return rc;
  }
  unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
  long long *nt = static_cast<long long *>(e->hs_t.p);
  unsigned long long *ns = static_cast<unsigned long long *>(e->hs_sorted.p);
  unsigned long long *koff = static_cast<unsigned long long *>(e->hs_koff.p), *coff = koff + kpad + 4;
  uint32_t *kcnt = static_cast<uint32_t *>(e->hs_kcnt.p);
  unsigned int *long_count = reinterpret_cast<unsigned int *>(kcnt + kpad);
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const unsigned long long *poff, *nv;
  batch_points(e, g, L, sparse_poff, P, &poff, &nv);   // 1.
  if (st->history) {   // 2. every key's new values sorted; 3. merged with its history into the candidate arena
    launch_hist_sort(s, nv, poff, K, ns, kcnt, long_count);
    launch_hist_merge(s, K, st->hist.off[cur], st->hist.val.p[cur], poff, ns, st->hist.off[cand], st->hist.val.p[cand], kcnt, coff, scratch,
                      hist_merge_chunks_bound(K, need));
  }
  if (st->series)      // 3'. appended to its series in the candidate arena
    launch_series_append(s, K, st->ser.off[cur], st->ser.val.p[cur], poff, nv, st->ser.off[cand], st->ser.val.p[cand]);
  if (st->times)       // 3''. and their times beside them (the same offsets, written again)
    launch_series_append(s, K, st->ser.off[cur], reinterpret_cast<const unsigned long long *>(st->ser_times.p[cur]), poff,
                         reinterpret_cast<const unsigned long long *>(nt), st->ser.off[cand], reinterpret_cast<unsigned long long *>(st->ser_times.p[cand]));
  HIP_TRY(e, hipMemcpyAsync(static_cast<unsigned char *>(e->counters.p) + kTailHistLen, poff + K, 8, hipMemcpyDeviceToDevice, s));
  hb->nk = nk; hb->nt = nt; hb->nv = nv; hb->poff = poff; hb->P_dev = poff + K; hb->P_cap = P_cap;
  if (dbscan && P_cap) {   // 4. verdicts of the new points; 5. their rows (the row total lands in the job's tail)
    uint8_t *noise = static_cast<uint8_t *>(e->hs_noise.p);
    uint32_t *cnt = static_cast<uint32_t *>(e->hs_cnt.p);
    unsigned long long *row = static_cast<unsigned long long *>(e->hs_row.p);
    launch_hist_verdict(s, nk, nv, poff + K, P_cap, st->hist.off[cand], st->hist.val.p[cand], jp.eps, jp.min_samples, jp.all_points, noise, cnt);
    launch_scan(s, cnt, row, P_cap, scratch, dev_total(e));
    hb->noise = noise; hb->cnt = cnt; hb->row = row;
  }
  return TAD_OK;
}

// One tad_state_merge batch (tad.h; kernels in tad_merge.hip), in the place of a stream batch's count pass: the batch's points in (key, time)
// order are classified against the current series, then either appended as a stream batch appends them (nothing inserted, combined or
// too old) or merged by time into the candidate series, times, history and moments.  Writes candidate memory and context workspace only;
// mc->changed tells run_job_locked whether the candidates are to become current.  One host round trip: the Stage-0 error word and the
// classification's counters; a Stage-0 error leaves the rest undone (run_job_locked retries or reports it).
int state_merge_batch(JobCtx *e, tad_state *st, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, uint64_t P_bound, bool op_max,
                      double alpha, MergeCall *mc) {
  hipStream_t s = e->stream;
  const uint64_t K = g.K;
  const int cur = st->cur, cand = cur ^ 1;
  const uint64_t P_cap = sparse_poff ? P : P_bound;
  const uint64_t pc = P_cap ? P_cap : 1;
  const size_t kpad = (size_t)((K + 3) & ~3ull), ko = kpad + 4;
  const uint64_t S = st->ser.len[cur], H = st->hist.len[cur];
  int rc;
  mc->changed = false;
  mc->added = 0;
  // the candidate arenas first: an allocation failure leaves the state as it is
  if ((rc = state_grow_candidates(e, st, P_cap)) != TAD_OK) return rc;
  if ((rc = ensure_batch_points(e, K, P_cap, sparse_poff != nullptr)) != TAD_OK) return rc;
  // per point: three scans (pc + 1 each) | history gains, sorted | losses, sorted | rank, three flag arrays | class
  if ((rc = ensure(e, e->mg_pts, (7 * pc + 8) * 8 + pc * 16 + pc + 64)) != TAD_OK) return rc;
  // per key: counters | long-list length | five offset arrays (K + 1 each) | four u32 arrays
  if ((rc = ensure(e, e->mg_keys, 128 + ko * 40 + kpad * 16)) != TAD_OK) return rc;
  unsigned long long *nhoff = static_cast<unsigned long long *>(e->mg_pts.p), *aoff = nhoff + pc + 2, *roff = aoff + pc + 2;
  unsigned long long *hadd = roff + pc + 2, *hadd_s = hadd + pc, *hrem = hadd_s + pc, *hrem_s = hrem + pc;
  uint32_t *rank = reinterpret_cast<uint32_t *>(hrem_s + pc), *f_nh = rank + pc, *f_kept = f_nh + pc, *f_hit = f_kept + pc;
  uint8_t *cls = reinterpret_cast<uint8_t *>(f_hit + pc);
  MergeCounters *mcnt = static_cast<MergeCounters *>(e->mg_keys.p);
  unsigned int *long_count = reinterpret_cast<unsigned int *>(mcnt + 1);
  unsigned long long *akoff = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->mg_keys.p) + 128), *rkoff = akoff + ko;
  unsigned long long *hoff_mid = rkoff + ko, *coff_s = hoff_mid + ko, *coff_h = coff_s + ko;
  uint32_t *chunks_s = reinterpret_cast<uint32_t *>(coff_h + ko), *chunks_h = chunks_s + kpad, *replay = chunks_h + kpad, *long_list = replay + kpad;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const unsigned long long *nk = static_cast<const unsigned long long *>(e->hs_key.p);
  const long long *nt = static_cast<const long long *>(e->hs_t.p);
  const unsigned long long *poff, *nv;
  batch_points(e, g, L, sparse_poff, P, &poff, &nv);
  // 1. classify; the one round trip: Stage 0's error word, the point count, the classification's counters
  HIP_TRY(e, hipMemsetAsync(mcnt, 0, sizeof(MergeCounters), s));
  launch_merge_classify(s, nk, nt, poff + K, P_cap, K, st->ser.off[cur], st->ser_times.p[cur], (long long)mc->keep_from, cls, rank, f_nh, f_kept, f_hit, mcnt);
  unsigned char *hm = e->tail_host + kTailMoments;   // (the moment partials' place in the pinned tail: a merge has none)
  HIP_TRY(e, hipMemcpyAsync(e->ctr_host, e->counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(hm, mcnt, sizeof(MergeCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(hm + sizeof(MergeCounters), poff + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  if (e->ctr_host->err != 0) return TAD_OK;
  MergeCounters c;
  unsigned long long points = 0;
  memcpy(&c, hm, sizeof c);
  memcpy(&points, hm + sizeof c, 8);
  tad_merge_stats &ms = mc->stats;
  ms.batch_points = points;
  ms.points_too_old = c.too_old;
  ms.points_appended = c.appended;
  ms.points_inserted = c.inserted;
  ms.points_combined = c.combined;
  ms.keys_touched = ms.keys_replayed = 0;
  if (c.appended + c.inserted + c.combined == 0) return TAD_OK;   // nothing to merge: the state stays as it is
  if (c.inserted == 0 && c.combined == 0 && c.too_old == 0) {
    // 6. every point is newer than what its key held: the append path of a stream batch (stream_history_batch's steps 2, 3, 3', 3'')
    if (st->history) {
      unsigned long long *ns = static_cast<unsigned long long *>(e->hs_sorted.p);
      launch_hist_sort(s, nv, poff, K, ns, long_list, long_count);
      launch_hist_merge(s, K, st->hist.off[cur], st->hist.val.p[cur], poff, ns, st->hist.off[cand], st->hist.val.p[cand], chunks_h, coff_h, scratch,
                        hist_merge_chunks_bound(K, H + P_cap));
    }
    launch_series_append(s, K, st->ser.off[cur], st->ser.val.p[cur], poff, nv, st->ser.off[cand], st->ser.val.p[cand]);
    launch_series_append(s, K, st->ser.off[cur], reinterpret_cast<const unsigned long long *>(st->ser_times.p[cur]), poff,
                         reinterpret_cast<const unsigned long long *>(nt), st->ser.off[cand], reinterpret_cast<unsigned long long *>(st->ser_times.p[cand]));
    launch_merge_moments(s, K, nullptr, st->ser.off[cur], st->ser.off[cand], st->ser.val.p[cand], st->ser_times.p[cand], alpha, state_view(st, cur),
                         state_view(st, cand), mcnt);
  } else {
    if (st->history && c.combined && (rc = ensure(e, e->mg_hist, (H ? H : 1) * 8)) != TAD_OK) return rc;
    // 2. the scans; per key: candidate offsets, the history's packed gains / losses, chunk counts, who replays
    launch_scan(s, f_nh, nhoff, P_cap, scratch);
    launch_scan(s, f_kept, aoff, P_cap, scratch);
    launch_scan(s, f_hit, roff, P_cap, scratch);
    launch_merge_keys(s, K, poff, nhoff, aoff, roff, cls, st->ser.off[cur], st->history ? st->hist.off[cur] : nullptr, st->ser.off[cand], akoff, rkoff,
                      hoff_mid, chunks_s, chunks_h, replay);
    launch_scan(s, chunks_s, coff_s, K, scratch);
    // 3. series and times merged by time (and the history's gains and losses packed)
    launch_merge_series(s, merge_chunks_bound(K, S + P_cap), coff_s, K, op_max, st->ser.off[cur], st->ser.val.p[cur], st->ser_times.p[cur], poff, nt, nv, cls, rank,
                        nhoff, aoff, roff, st->ser.off[cand], st->ser.val.p[cand], st->ser_times.p[cand], st->history ? hadd : nullptr, st->history ? hrem : nullptr);
    if (st->history) {   // 4. the combined points' old values leave the history (through the scratch arena), then the batch's values enter
      const unsigned long long *hoff_from = st->hist.off[cur], *hval_from = st->hist.val.p[cur];
      if (c.combined) {
        unsigned long long *hmid = static_cast<unsigned long long *>(e->mg_hist.p);
        launch_hist_sort(s, hrem, rkoff, K, hrem_s, long_list, long_count);
        launch_scan(s, chunks_h, coff_h, K, scratch);
        // (chunks_h gives an empty key no chunk: not the one-chunk-at-least counts of a trim)
        launch_hist_subtract(s, trim_chunks_bound(K, H), coff_h, K, st->hist.off[cur], st->hist.val.p[cur], rkoff, hrem_s, hoff_mid, hmid, false);
        hoff_from = hoff_mid;
        hval_from = hmid;
      }
      launch_hist_sort(s, hadd, akoff, K, hadd_s, long_list, long_count);
      launch_hist_merge(s, K, hoff_from, hval_from, akoff, hadd_s, st->hist.off[cand], st->hist.val.p[cand], chunks_h, coff_h, scratch,
                        hist_merge_chunks_bound(K, H + P_cap));
    }
    // 5. the moments
    launch_merge_moments(s, K, replay, st->ser.off[cur], st->ser.off[cand], st->ser.val.p[cand], st->ser_times.p[cand], alpha, state_view(st, cur),
                         state_view(st, cand), mcnt);
  }
  HIP_TRY(e, hipMemcpyAsync(hm, mcnt, sizeof(MergeCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  memcpy(&c, hm, sizeof c);
  ms.keys_touched = c.keys_touched;
  ms.keys_replayed = c.keys_replayed;
  mc->changed = true;
  mc->added = c.inserted + c.appended;
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
  const size_t kpad = (size_t)((K + 3) & ~3ull);
  int rc;
  // per key: touched u32 | len8 u32 | tidx u64[K + 1] | yoffk u64[K + 1] | tmax; per slot: key u32 | lo u32 | hi u32 | ok u8 | yoff u64 | lam | sigma | ibase
  if ((rc = ensure(e, e->as_key, kpad * 8 + (kpad + 4) * 16 + 64 + kpad * (4 * 3 + 1 + 8 * 4) + 256)) != TAD_OK) return rc;
  unsigned char *kb = static_cast<unsigned char *>(e->as_key.p);
  uint32_t *touched = reinterpret_cast<uint32_t *>(kb), *len8 = touched + kpad;
  unsigned long long *tidx = reinterpret_cast<unsigned long long *>(len8 + kpad), *yoffk = tidx + kpad + 4;
  unsigned int *tmax_dev = reinterpret_cast<unsigned int *>(yoffk + kpad + 4);
  unsigned char *sb = reinterpret_cast<unsigned char *>(tmax_dev) + 64;
  ArimaSlots sl;
  sl.yoff = reinterpret_cast<unsigned long long *>(sb);
  sl.lam = reinterpret_cast<double *>(sl.yoff + kpad);
  sl.sigma = sl.lam + kpad;
  sl.ibase = reinterpret_cast<unsigned long long *>(sl.sigma + kpad);
  sl.key = reinterpret_cast<uint32_t *>(sl.ibase + kpad);
  sl.lo = sl.key + kpad;
  sl.hi = sl.lo + kpad;
  sl.ok = reinterpret_cast<uint8_t *>(sl.hi + kpad);
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  launch_as_touch(s, K, soff, hb.poff, touched, len8, tmax_dev);
  launch_scan(s, touched, tidx, K, scratch);
  launch_scan(s, len8, yoffk, K, scratch);
  unsigned long long hv[3] = {0, 0, 0};   // new points, slots, packed doubles
  unsigned int tmax = 0;
  HIP_TRY(e, hipMemcpyAsync(&hv[0], hb.P_dev, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&hv[1], tidx + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&hv[2], yoffk + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(&tmax, tmax_dev, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(e->ctr_host, ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  const uint64_t P = hv[0], Kt = hv[1], S8 = hv[2];
  ab->P = 0;
  if (e->ctr_host->err != 0 || P == 0) return TAD_OK;   // (the caller reads the error from the tail)
  // per new point: pcalc f64 | rows u32 | row_off u64[P + 1] | pflag u8; the packed series: lx | ysk, each with the slack an idle lane's
  // staged loads (k_arima_fit_list reads slot 0's offset up to the wavefront's position + 16) may touch
  const size_t ppad = (size_t)((P + 3) & ~3ull);
  if ((rc = ensure(e, e->as_pt, ppad * (8 + 4 + 8 + 1) + 64)) != TAD_OK) return rc;
  double *pcalc = static_cast<double *>(e->as_pt.p);
  uint32_t *rows = reinterpret_cast<uint32_t *>(pcalc + ppad);
  unsigned long long *row_off = reinterpret_cast<unsigned long long *>(rows + ppad);
  uint8_t *pflag = reinterpret_cast<uint8_t *>(row_off + ppad + 4);
  const size_t ser = (size_t)S8 + tmax + 32;
  if ((rc = ensure(e, e->as_ser, ser * 16)) != TAD_OK) return rc;
  double *lx = static_cast<double *>(e->as_ser.p), *ysk = lx + ser;
  HIP_TRY(e, hipMemsetAsync(pflag, 0, P, s));
  HIP_TRY(e, hipMemsetAsync(ysk, 0, ser * 8, s));   // (the slack: finite values for idle lanes)
  launch_as_prep(s, K, soff, sval, hb.poff, v.mom, tidx, yoffk, lx, ysk, sl, pcalc, pflag, ctr);
  // the fits: counted per position, listed, their wavefronts laid out on the host (heaviest position first)
  const uint64_t npos = (uint64_t)tmax + 1;
  if ((rc = ensure(e, e->as_pos, npos * (4 + 8) + 128)) != TAD_OK) return rc;   // cnt u32[npos] | (64-byte aligned) loff u64[npos + 1]
  unsigned int *pcnt = static_cast<unsigned int *>(e->as_pos.p);
  unsigned long long *loff = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->as_pos.p) + ((npos * 4 + 63) & ~63ull));
  HIP_TRY(e, hipMemsetAsync(pcnt, 0, npos * 4, s));
  launch_as_list(s, Kt, sl, false, pcnt, nullptr, nullptr, nullptr);
  std::vector<uint32_t> hcnt;
  std::vector<unsigned long long> hoff;
  std::vector<uint32_t> wave_pos;
  try { hcnt.resize(npos); hoff.resize(npos + 1); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  HIP_TRY(e, hipMemcpyAsync(hcnt.data(), pcnt, npos * 4, hipMemcpyDeviceToHost, s));
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
  const size_t fpad = (size_t)((nfits + 3) & ~3ull);
  if ((rc = ensure(e, e->as_fit, fpad * 8 + (size_t)(waves + 4) * 4 + 64)) != TAD_OK) return rc;
  uint32_t *list = static_cast<uint32_t *>(e->as_fit.p), *fpos = list + fpad, *wpos = fpos + fpad;
  if (nfits) {
    HIP_TRY(e, hipMemcpyAsync(loff, hoff.data(), (npos + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemcpyAsync(wpos, wave_pos.data(), waves * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemsetAsync(pcnt, 0, npos * 4, s));
    launch_as_list(s, Kt, sl, true, pcnt, loff, list, fpos);
    const size_t wsb = arima_stream_ws_bytes(nfits, npos, waves);
    if ((rc = ensure(e, e->as_ws, wsb)) != TAD_OK) return rc;
    const FitListArgs fa{wpos, pcnt, loff, list, hb.nv, pcalc, pflag};
    // the fit yields to whole-CU jobs of other contexts like tad_run's (arima_yield_loop); this job's own claim is dropped meanwhile
    const bool held = e->hold && e->hold->held;
    if (held) e->hold->release();
    const unsigned int *yielded_dev = nullptr;
    if (launch_arima_stream_fit(s, true, nfits, npos, waves, fpos, ysk, sl, fa, jp.maxiter, ctr, e->as_ws.p, e->eng->pause_dev, &yielded_dev, 0) != 0)
      return fail(e, TAD_ERR_HIP, "ARIMA launch failed");
    if ((rc = arima_yield_loop(e, yielded_dev, [&](uint32_t grace, const unsigned int **yd) {
           return launch_arima_stream_fit(s, false, nfits, npos, waves, fpos, ysk, sl, fa, jp.maxiter, ctr, e->as_ws.p, e->eng->pause_dev, yd, grace);
         })) != TAD_OK)
      return rc;
    if (held) e->hold->acquire();
  }
  // rows of the new points (the row total lands in the job's tail)
  launch_as_rows(s, P, hb.nk, tidx, sl.ok, pflag, jp.all_points, rows);
  launch_scan(s, rows, row_off, P, scratch, dev_total(e));
  ab->P = P; ab->tidx = tidx; ab->sigma = sl.sigma; ab->pcalc = pcalc; ab->pflag = pflag; ab->rows = rows; ab->row_off = row_off;
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
  if ((rc = ensure(e, e->ds_key, drop_state_key_bytes(K))) != TAD_OK) return rc;
  // per judged point: row u64[pc + 1] | cnt u32 | flag u8
  if ((rc = ensure(e, e->ds_pt, (pc + 1) * 8 + pc * 4 + pc + 64)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > pc ? K : pc) * sizeof(unsigned long long))) != TAD_OK) return rc;
  const DropStateKeys dk = drop_state_keys(e->ds_key.p, K);
  unsigned long long *row = static_cast<unsigned long long *>(e->ds_pt.p);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(row + pc + 1);
  uint8_t *flag = reinterpret_cast<uint8_t *>(cnt + pc);
  if (touched_only) launch_ds_route(s, K, v.soff, hb.poff, coop_min, list, lcount);
  launch_ds_stats(s, K, v.soff, v.sval, touched_only ? hb.poff : nullptr, coop_min, list, lcount, jp.drop_min_samples, dk, ctr);
  if (!touched_only) launch_moments(s, K, dk.n, dk.mean, dk.m2, dev_moments(e), ctr);   // (and n_keys / n_points)
  if (hb.P_cap) {
    launch_ds_verdict(s, hb.nk, hb.nv, hb.P_dev, hb.P_cap, dk, jp.drop_nsigma, jp.all_points, flag, cnt);
    launch_scan(s, cnt, row, hb.P_cap, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
  }
  db->keys = dk; db->flag = flag; db->cnt = cnt; db->row = row;
  return TAD_OK;
}

// the start of a tad_run_state / tad_run_state_window job on the context the caller holds: progress, the first event, the job tail zeroed
static int run_view_begin(JobCtx *e, uint64_t K) {
  e->done.store(0);
  e->total.store(4);
  e->arima_relaunches = 0;
  int rc;
  if ((rc = ensure_key_buffers(e, K)) != TAD_OK) return rc;
  HIP_TRY(e, hipEventRecord(e->ev[0], e->stream));
  HIP_TRY(e, hipMemsetAsync(e->counters.p, 0, kTailBytes, e->stream));
  return TAD_OK;
}

// tad_run_state / tad_run_state_window after run_view_begin (tad.h; kernels: tad_window.hip).  Reads the view only: the state's CURRENT
// copies, or a window's view in this context's workspace (wv_key / wv_pts, which nothing below resizes).  EWMA walks the CSR series;
// DBSCAN, ARIMA and DROP (tad_drop_state: its view carries no moments) run the stream's kernels with every series point named as new
// (poff = the series offsets).  view_syncs: the host synchronisations the caller spent on building the view (tad_stats.host_syncs).
static int run_view_locked(JobCtx *e, const StateView &v, const tad_job *job, tad_mem out_memory, tad_result **out, int view_syncs) {
  hipStream_t s = e->stream;
  JobParams jp = job_params(job);
  const uint64_t K = v.K;
  const uint64_t P = v.P;
  const unsigned long long *soff = v.soff, *sval = v.sval;
  const long long *stt = v.st;
  const StreamState view = v.mom;
  int rc;
  DevCounters *ctr = static_cast<DevCounters *>(e->counters.p);
  unsigned long long *tmin_dev = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->counters.p) + kTailHistLen);
  uint64_t rows = 0;
  HistBatch hist;
  ArimaBatch ab;
  DropBatch db;
  const bool ewma = jp.algo == TAD_ALGO_EWMA;
  unsigned long long coop_min = 0;
  uint32_t *list = nullptr;
  unsigned int *lcount = nullptr;
  const unsigned long long *off = soff;   // EWMA with every point: the row offsets are the series offsets
  if (P) {
    const size_t kpad = (size_t)((K + 3) & ~3ull);
    if ((rc = ensure(e, e->hs_kcnt, kpad * 4 + 64)) != TAD_OK) return rc;   // the long keys' list | its length
    if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > P ? K : P) * sizeof(unsigned long long))) != TAD_OK) return rc;
    list = static_cast<uint32_t *>(e->hs_kcnt.p);
    lcount = reinterpret_cast<unsigned int *>(list + kpad);
    unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
    coop_min = win_coop_min(K, P);
    launch_win_route(s, K, soff, stt, coop_min, list, lcount, tmin_dev);
    if (jp.algo != TAD_ALGO_DROP) launch_moments(s, K, view.n, view.avg, view.m2, dev_moments(e), ctr);   // (and n_keys / n_points)
    if (ewma) {
      if (!jp.all_points) {
        launch_win_ewma(s, K, soff, sval, stt, view, jp.alpha, coop_min, list, lcount, false, false, static_cast<uint32_t *>(e->n_anom.p), nullptr, OutRows{});
        launch_scan(s, static_cast<const uint32_t *>(e->n_anom.p), static_cast<unsigned long long *>(e->off.p), K, scratch, dev_total(e));
        off = static_cast<const unsigned long long *>(e->off.p);
      }
    } else {
      if ((rc = ensure(e, e->hs_key, P * 8)) != TAD_OK) return rc;
      unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
      launch_win_keys(s, K, soff, nk);
      hist.nk = nk; hist.nv = sval; hist.nt = stt; hist.poff = soff; hist.P_dev = soff + K; hist.P_cap = P;
      if (jp.algo == TAD_ALGO_DBSCAN) {
        if ((rc = ensure(e, e->hs_noise, P)) != TAD_OK) return rc;
        if ((rc = ensure(e, e->hs_cnt, P * 4)) != TAD_OK) return rc;
        if ((rc = ensure(e, e->hs_row, (P + 1) * 8)) != TAD_OK) return rc;
        uint8_t *noise = static_cast<uint8_t *>(e->hs_noise.p);
        uint32_t *cnt = static_cast<uint32_t *>(e->hs_cnt.p);
        unsigned long long *row = static_cast<unsigned long long *>(e->hs_row.p);
        launch_hist_verdict(s, nk, sval, hist.P_dev, P, v.hoff, v.hval, jp.eps, jp.min_samples, jp.all_points, noise, cnt);
        launch_scan(s, cnt, row, P, scratch, dev_total(e));
        hist.noise = noise; hist.cnt = cnt; hist.row = row;
      } else if (jp.algo == TAD_ALGO_DROP) {
        if ((rc = state_drop_batch(e, v, hist, jp, false, coop_min, list, lcount, ctr, &db)) != TAD_OK) return rc;
      } else if ((rc = stream_arima_batch(e, v, hist, jp, ctr, &ab)) != TAD_OK) {
        return rc;
      }
    }
  }
  e->done.store(2);
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  rows = (ewma && jp.all_points) ? P : (P ? *e->total_host : 0);
  const DevCounters c = *e->ctr_host;
  e->done.store(3);

  RowsOut ro;
  if ((rc = make_result(e, rows, jp.all_points, out_memory, &ro.rp, &ro.dev_rows, &ro.dev_block)) != TAD_OK) return rc;
  const OutRows dev_rows = ro.dev_rows;
  if (rows && ewma)
    launch_win_ewma(s, K, soff, sval, stt, view, jp.alpha, coop_min, list, lcount, true, jp.all_points, nullptr, off, dev_rows, rows, e->plan.ewma_emit,
                    e->plan.ewma_emit_rows);
  else if (rows && jp.algo == TAD_ALGO_DBSCAN)
    launch_hist_emit(s, hist.nk, hist.nt, hist.nv, hist.P_dev, hist.P_cap, hist.noise, hist.cnt, hist.row, view, jp.all_points, dev_rows);
  else if (rows && jp.algo == TAD_ALGO_DROP)
    launch_ds_emit(s, hist.nk, hist.nt, hist.nv, hist.P_dev, hist.P_cap, db.flag, db.cnt, db.row, db.keys, jp.all_points, dev_rows);
  else if (rows)
    launch_as_emit(s, ab.P, hist.nk, hist.nt, hist.nv, ab.tidx, ab.sigma, ab.pcalc, ab.pflag, ab.rows, ab.row_off, jp.all_points, dev_rows);
  if ((rc = finish_rows(e, job, &ro, rows, jp.all_points, c, P != 0)) != TAD_OK) return rc;
  tad_stats &rs = ro.rp->pub.stats;
  rs.rows_in = rs.rows_used = rs.n_points = P;
  {
    unsigned long long tmin = ~0ull;
    memcpy(&tmin, e->tail_host + kTailHistLen, 8);
    rs.t0 = (P && tmin != ~0ull) ? (int64_t)(tmin ^ (1ull << 63)) : 0;
  }
  hipEventElapsedTime(&rs.ms_total, e->ev[0], e->ev[4]);
  rs.ms_detect = rs.ms_total;   // no Stage 0 ran: the whole call is the detector and its emit
  rs.host_syncs = 2 + view_syncs;
  e->done.store(4);
  *out = &ro.rp->pub;
  return TAD_OK;
}

}  // namespace tadh

extern "C" {

// what tad_run_state and tad_run_state_window refuse before they take the state's lock (who: the call's name for the message)
static int check_state_job(tad_engine *eng, const tad_state *st, const tad_job *job, tad_result **out, const char *who, const char *narrow) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and out must not be NULL", who);
  *out = nullptr;
  if (job->algo != TAD_ALGO_EWMA && job->algo != TAD_ALGO_DBSCAN && job->algo != TAD_ALGO_ARIMA)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be EWMA, DBSCAN or ARIMA (DROP: tad_drop_state)", who);
  if (job->start_time != 0 || job->end_time != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: start_time / end_time must be 0: %s", who, narrow);
  if (job->flags & (TAD_FLAG_KEY_U32 | TAD_FLAG_TIME_U32))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 describe input columns; there are none", who);
  if (job->ewma_alpha < 0.0 || job->ewma_alpha > 1.0 || job->dbscan_eps < 0.0 || job->dbscan_min_samples < 0 || job->arima_maxiter < 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: detector parameter out of range", who);
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES)", who);
  if (job->algo == TAD_ALGO_DBSCAN && !st->history)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: DBSCAN needs a state with history too (TAD_STATE_HISTORY)", who);
  return TAD_OK;
}

int tad_run_state(tad_engine *eng, tad_state *st, const tad_job *job, tad_mem out_memory, tad_result **out) {
  int rc = check_state_job(eng, st, job, out, "tad_run_state", "the window is what the state holds (tad_state_trim narrows it)");
  if (rc != TAD_OK) return rc;
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_run_state: the series was imported without its times (tad_state_import_times)");
  if ((rc = call.enter("tad_run_state", job->id, job->algo == TAD_ALGO_ARIMA)) != TAD_OK) return rc;
  if ((rc = run_view_begin(call.e, st->K)) != TAD_OK) return rc;
  return run_view_locked(call.e, series_view(st, st->cur), job, out_memory, out, 0);
}

int tad_window_history_by_sort(uint64_t window_points, uint64_t state_points) { return win_hist_by_sort(window_points, state_points) ? 1 : 0; }

// The view of a window of the state in the context's workspace (kernels: tad_window.hip), after run_view_begin, in two steps that
// tad_run_state_window and tad_drop_state share: window_bounds (every key's bounds, the view's offsets, the window's point total — one
// host round trip) and window_gather (the view itself, which run_view_locked then judges).  Both read the state's CURRENT copies and
// write workspace only: wv_key and wv_pts hold the view; run_view_locked resizes neither.
struct WinKeys {   // wv_key: per key wbeg | wlen | ecnt | chunks (later the long-sort list) u32 each | the list's length | woff | coff | eoff u64[K + 1] each | moments
  uint32_t *wbeg, *wlen, *ecnt, *chunks;
  unsigned int *long_count;
  unsigned long long *woff, *coff, *eoff;
  StreamState wmom;
};

static size_t win_key_bytes(uint64_t K) {
  const size_t kpad = (size_t)((K + 3) & ~3ull);
  return kpad * 16 + 64 + (kpad + 4) * 24;
}

static WinKeys win_keys(JobCtx *e, uint64_t K) {
  const size_t kpad = (size_t)((K + 3) & ~3ull);
  WinKeys w;
  w.wbeg = static_cast<uint32_t *>(e->wv_key.p); w.wlen = w.wbeg + kpad; w.ecnt = w.wlen + kpad; w.chunks = w.ecnt + kpad;
  w.long_count = reinterpret_cast<unsigned int *>(w.chunks + kpad);
  w.woff = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>(w.long_count) + 64);
  w.coff = w.woff + kpad + 4; w.eoff = w.coff + kpad + 4;
  w.wmom = stream_view(static_cast<unsigned char *>(e->wv_key.p) + win_key_bytes(K), K);
  return w;
}

// 1. every key's bounds; the view's offsets and the chunk offsets; *P = the window's point total.  keep (device, K bytes, or NULL): the
// key selection of tad_run_state_keys / tad_drop_state_keys — a key that is not selected gets an empty window
static int window_bounds(JobCtx *e, const tad_state *st, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *keep, uint64_t *P) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const StateView whole = series_view(st, st->cur);
  int rc;
  if ((rc = ensure(e, e->wv_key, win_key_bytes(K) + state_bytes(K))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K) * sizeof(unsigned long long))) != TAD_OK) return rc;
  const WinKeys w = win_keys(e, K);
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  launch_win_bounds(s, K, whole.soff, whole.st, (long long)from_t, (long long)to_t, keep_points, keep, w.wbeg, w.wlen, w.ecnt, w.chunks);
  launch_scan(s, w.wlen, w.woff, K, scratch);
  launch_scan(s, w.chunks, w.coff, K, scratch);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(e->tail_host + kTailTotal, w.woff + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  *P = *e->total_host;
  return TAD_OK;
}

// 2. the window's values and times (DBSCAN on the subtract side: the excluded values too); 3. the moments — not for TAD_ALGO_DROP, which
// reads none; 4. DBSCAN's history, by sorting the window's values or (subtract) by removing the sorted excluded values from the state's
static int window_gather(JobCtx *e, const tad_state *st, const tad_job *job, uint64_t P, bool subtract, StateView *v) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  const WinKeys w = win_keys(e, K);
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  int rc;
  *v = StateView{};
  v->K = K;
  v->P = P;
  if (P != 0) {
    const bool dbscan = job->algo == TAD_ALGO_DBSCAN;
    if ((rc = ensure(e, e->wv_pts, P * (dbscan ? 24 : 16))) != TAD_OK) return rc;
    unsigned long long *wval = static_cast<unsigned long long *>(e->wv_pts.p);
    long long *wt = reinterpret_cast<long long *>(wval + P);
    unsigned long long *wh = wval + 2 * P, *ev = nullptr, *es = nullptr;
    if (subtract) {
      if ((rc = ensure(e, e->hs_val, (S - P) * 8)) != TAD_OK) return rc;
      if ((rc = ensure(e, e->hs_sorted, (S - P) * 8)) != TAD_OK) return rc;
      ev = static_cast<unsigned long long *>(e->hs_val.p);
      es = static_cast<unsigned long long *>(e->hs_sorted.p);
      launch_scan(s, w.ecnt, w.eoff, K, scratch);
    }
    const uint64_t bound = trim_chunks_bound(K, S);
    launch_win_gather(s, bound, w.coff, K, whole.soff, whole.sval, whole.st, w.wbeg, w.woff, wval, wt, w.eoff, ev);
    if (job->algo != TAD_ALGO_DROP) {
      const double alpha = job->ewma_alpha == 0.0 ? 0.5 : job->ewma_alpha;   // (for the view's ewma only, which no detector reads)
      launch_trim_moments(s, K, w.wlen, w.ecnt, w.woff, wval, alpha, whole.mom, w.wmom);
    }
    if (subtract) {
      launch_hist_sort(s, ev, w.eoff, K, es, w.chunks, w.long_count);
      launch_hist_subtract(s, bound, w.coff, K, whole.hoff, whole.hval, w.eoff, es, w.woff, wh, true);
    } else if (dbscan) {
      launch_hist_sort(s, wval, w.woff, K, wh, w.chunks, w.long_count);
    }
    HIP_TRY(e, hipGetLastError());
    v->soff = w.woff; v->sval = wval; v->st = wt; v->mom = w.wmom;
    if (dbscan) { v->hoff = w.woff; v->hval = wh; }
  }
  e->done.store(1);
  return TAD_OK;
}

// tad.h: the window's view (window_bounds, window_gather), then tad_run_state's path on it.
int tad_run_state_window(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, tad_mem out_memory,
                         tad_result **out) {
  int rc = check_state_job(eng, st, job, out, "tad_run_state_window", "the window is from_t / to_t / keep_points");
  if (rc != TAD_OK) return rc;
  if (from_t != 0 && to_t != 0 && from_t > to_t)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_run_state_window: from_t is later than to_t");
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_run_state_window: the series was imported without its times (tad_state_import_times)");
  if ((rc = call.enter("tad_run_state_window", job->id, job->algo == TAD_ALGO_ARIMA)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  if ((rc = run_view_begin(e, st->K)) != TAD_OK) return rc;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  if (S == 0 || (from_t == 0 && to_t == 0 && keep_points == 0)) return run_view_locked(e, whole, job, out_memory, out, 0);
  uint64_t P = 0;
  if ((rc = window_bounds(e, st, from_t, to_t, keep_points, nullptr, &P)) != TAD_OK) return rc;
  if (P == S) return run_view_locked(e, whole, job, out_memory, out, 1);   // every key is whole: the state's own arrays, no view
  const bool subtract = job->algo == TAD_ALGO_DBSCAN && P != 0 && !win_hist_by_sort(P, S);
  StateView v;
  if ((rc = window_gather(e, st, job, P, subtract, &v)) != TAD_OK) return rc;
  return run_view_locked(e, v, job, out_memory, out, 1);
}

// tad.h: the drop detector's batch verdicts over a window of the state — tad_run_state_window's window and view (window_bounds, window_gather:
// values and times only), then run_view_locked's DROP path (state_drop_batch).  Read-only.
int tad_drop_state(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, tad_mem out_memory,
                   tad_result **out) {
  const char *who = "tad_drop_state";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and out must not be NULL", who);
  *out = nullptr;
  if (job->algo != TAD_ALGO_DROP)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be DROP (tad_run_state_window judges EWMA, DBSCAN and ARIMA)", who);
  if (job->start_time != 0 || job->end_time != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: start_time / end_time must be 0: the window is from_t / to_t / keep_points", who);
  if (job->flags & (TAD_FLAG_KEY_U32 | TAD_FLAG_TIME_U32))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 describe input columns; there are none", who);
  if (!(job->drop_nsigma >= 0.0) || job->drop_min_samples < 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: detector parameter out of range", who);
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES)", who);
  if (from_t != 0 && to_t != 0 && from_t > to_t) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: from_t is later than to_t", who);
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times)", who);
  int rc;
  if ((rc = call.enter(who, job->id)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  if ((rc = run_view_begin(e, st->K)) != TAD_OK) return rc;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  if (S == 0 || (from_t == 0 && to_t == 0 && keep_points == 0)) return run_view_locked(e, whole, job, out_memory, out, 0);
  uint64_t P = 0;
  if ((rc = window_bounds(e, st, from_t, to_t, keep_points, nullptr, &P)) != TAD_OK) return rc;
  if (P == S) return run_view_locked(e, whole, job, out_memory, out, 1);   // every key is whole: the state's own arrays, no view
  StateView v;
  if ((rc = window_gather(e, st, job, P, false, &v)) != TAD_OK) return rc;   // values and times only: DROP reads no moments, no history
  return run_view_locked(e, v, job, out_memory, out, 1);
}

// tad.h: tad_run_state_window / tad_drop_state over the keys key_keep selects, once the job is checked (the window calls' own checks, under
// the *_keys name).  A key whose byte is 0 is left empty by window_bounds, and the rest of the call treats it as any key the window left
// empty.  The mask is a window of its own, so with one the "no window at all" shortcut is not taken; P == S still is, since then every
// point the state holds is selected.  Without a mask (NULL, length 0) this is the window call, step for step.  DROP: values and times only, no moments, no history.
static int window_keys_call(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *key_keep,
                            uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out, const char *who) {
  if (from_t != 0 && to_t != 0 && from_t > to_t) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: from_t is later than to_t", who);
  if (!key_keep && key_keep_len != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep is NULL with a length of %llu", who, (unsigned long long)key_keep_len);
  if (key_keep && key_memory != TAD_MEM_HOST && key_memory != TAD_MEM_DEVICE)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep must be in host or device memory", who);
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times)", who);
  if (key_keep && key_keep_len != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep has %llu entries, the state holds %llu keys", who, (unsigned long long)key_keep_len,
                (unsigned long long)st->K);
  int rc;
  if ((rc = call.enter(who, job->id, job->algo == TAD_ALGO_ARIMA)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  if ((rc = run_view_begin(e, st->K)) != TAD_OK) return rc;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  if (S == 0 || (!key_keep && from_t == 0 && to_t == 0 && keep_points == 0)) return run_view_locked(e, whole, job, out_memory, out, 0);
  const uint8_t *d_keep = key_keep;
  if (key_keep && key_memory == TAD_MEM_HOST) {   // staged: only window_bounds reads it
    if ((rc = ensure(e, e->in_key, (size_t)st->K)) != TAD_OK) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->in_key.p, key_keep, st->K, hipMemcpyHostToDevice, e->stream));
    d_keep = static_cast<const uint8_t *>(e->in_key.p);
  }
  uint64_t P = 0;
  if ((rc = window_bounds(e, st, from_t, to_t, keep_points, d_keep, &P)) != TAD_OK) return rc;
  if (P == S) return run_view_locked(e, whole, job, out_memory, out, 1);   // every key is selected and whole: the state's own arrays, no view
  const bool subtract = job->algo == TAD_ALGO_DBSCAN && P != 0 && !win_hist_by_sort(P, S);   // (P: the SELECTED window points)
  StateView v;
  if ((rc = window_gather(e, st, job, P, subtract, &v)) != TAD_OK) return rc;
  return run_view_locked(e, v, job, out_memory, out, 1);
}

int tad_run_state_keys(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *key_keep,
                       uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out) {
  const int rc = check_state_job(eng, st, job, out, "tad_run_state_keys", "the window is from_t / to_t / keep_points");
  if (rc != TAD_OK) return rc;
  return window_keys_call(eng, st, job, from_t, to_t, keep_points, key_keep, key_keep_len, key_memory, out_memory, out, "tad_run_state_keys");
}

int tad_drop_state_keys(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *key_keep,
                        uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out) {
  const char *who = "tad_drop_state_keys";
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and out must not be NULL", who);
  *out = nullptr;
  if (job->algo != TAD_ALGO_DROP)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be DROP (tad_run_state_keys judges EWMA, DBSCAN and ARIMA)", who);
  if (job->start_time != 0 || job->end_time != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: start_time / end_time must be 0: the window is from_t / to_t / keep_points", who);
  if (job->flags & (TAD_FLAG_KEY_U32 | TAD_FLAG_TIME_U32))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 describe input columns; there are none", who);
  if (!(job->drop_nsigma >= 0.0) || job->drop_min_samples < 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: detector parameter out of range", who);
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES)", who);
  return window_keys_call(eng, st, job, from_t, to_t, keep_points, key_keep, key_keep_len, key_memory, out_memory, out, who);
}

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

// tad.h: a batch placed by time.  The batch runs as a stream batch does up to the end of Stage 0 (run_job_locked with the context's merge
// mode set), then state_merge_batch.
int tad_state_merge(tad_engine *eng, tad_state *st, const tad_job *job, const tad_columns *cols, int64_t keep_from_t, tad_merge_stats *stats) {
  if (stats) memset(stats, 0, sizeof *stats);
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: engine is NULL");
  if (!st || !job || !cols) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: state, job and cols must not be NULL");
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES): "
                                               "without them it does not know where a late point belongs; state unchanged");
  if (job->flags & TAD_FLAG_EMIT_ALL_POINTS)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: TAD_FLAG_EMIT_ALL_POINTS asks for rows; a merge emits none (tad_run_state judges the window)");
  if (!(job->ewma_alpha >= 0.0 && job->ewma_alpha <= 1.0)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: ewma_alpha out of range");
  if (cols->num_keys != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: batch declares %llu keys, the state holds %llu (they must be equal)",
                (unsigned long long)cols->num_keys, (unsigned long long)st->K);
  {
    const int vrc = validate_job_columns(eng, job, cols, "tad_state_merge");
    if (vrc != TAD_OK) return vrc;
  }
  tad_job j = *job;   // the detector is not run: a stream batch of the EWMA kind up to the end of Stage 0
  j.algo = TAD_ALGO_EWMA;
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_merge: the series was imported without its times (tad_state_import_times); state unchanged");
  int rc = call.enter("tad_state_merge", j.id);
  if (rc != TAD_OK) return rc;
  PauseHold hold(eng);     // (declared after the call's context: dropped before the context goes back to the pool)
  call.e->hold = &hold;
  MergeCall mc;
  mc.keep_from = keep_from_t;
  call.e->merge = &mc;
  tad_result *none = nullptr;
  rc = run_job_locked(call.e, &j, cols, TAD_MEM_DEVICE, &none, nullptr, st, 0);
  call.e->merge = nullptr;
  if (rc == TAD_OK && stats) *stats = mc.stats;
  return rc;
}



}  // extern "C"