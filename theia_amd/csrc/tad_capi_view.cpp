// tad_capi_view.cpp — the read-only jobs on a streaming state of include/tad.h: tad_run_state, tad_run_state_window, tad_drop_state and
// their *_keys forms.  All five are one call (view_call): one checker for what they refuse, one window — time bounds, a point count, a key
// mask, any of them absent — whose view is built in the context's workspace (window_bounds, window_gather; kernels: tad_window.hip), and
// one job on that view (run_view_locked), which runs the stream batches' detectors (tad_capi.cpp) with every point of the view named as
// new.  tad_run_state_since / tad_drop_state_since are the same call with a Since: the view is judged whole, and only every key's points
// from a time on are named as new (the stream's own rule: a per-key suffix).  tad_run_state_buckets is the same call with three more
// fields of the window: the judged points are folded into time buckets (window_buckets in window_gather's place) and the view's points
// are the buckets.  Nothing here writes the state.
#include "tad_bucket.h"
#include "tad_engine.h"

using namespace tad;
using namespace tadh;

namespace {

// the start of a job on a view, on the context the caller holds: progress, the first event, the job tail zeroed
int run_view_begin(JobCtx *e, uint64_t K) {
  e->done.store(0);
  e->total.store(4);
  e->arima_relaunches = 0;
  int rc;
  if ((rc = ensure_key_buffers(e, K)) != TAD_OK) return rc;
  HIP_TRY(e, hipEventRecord(e->ev[0], e->stream));
  HIP_TRY(e, hipMemsetAsync(e->counters.p, 0, kTailBytes, e->stream));
  return TAD_OK;
}

// what run_view_locked's detectors leave for its emit, across the host round trip
struct ViewJob {
  HistBatch hist;
  ArimaBatch ab;
  DropBatch db;
  unsigned long long coop_min = 0;   // the routing launch_win_route left: keys from coop_min points on are on the list
  uint32_t *list = nullptr;
  unsigned int *lcount = nullptr;
  const unsigned long long *off = nullptr;   // EWMA: the row offsets
  const uint32_t *first = nullptr;           // EWMA with a Since: every key's first reported index
  int syncs = 0;                             // host round trips view_detect itself spent (a Since of DBSCAN, ARIMA and DROP: the reported total)
};

// tad_run_state_since / tad_drop_state_since: what is reported of the judged view — of key k the points with flow_end_s >= since_t (0: no
// such bound) and >= key_since[k] (device, K entries; NULL: no such bound).  keys: the call's per-key block in sn_key, carved by view_call
struct Since {
  const long long *key_since = nullptr;
  long long since_t = 0;
  SinceKeys keys{};
  long long bucket_s = 0, bucket_origin = 0;   // tad_run_state_buckets: the threshold is floored to its bucket's start (0: not bucketed)
};

// Before the round trip: the routing, the moments, the detector and its row total.  EWMA walks the CSR series; DBSCAN, ARIMA and DROP
// (its view carries no moments) run the stream's kernels with every series point named as new (poff = the series offsets).
// since != NULL: the reported points are a suffix of every key's segment (launch_win_since).  EWMA walks every series and counts or emits
// from first[k] on; the others get the suffixes packed as their batch of new points, after one more round trip for the packed total,
// and DROP judges the keys with a reported point only (touched_only, as a stream batch).
int view_detect(JobCtx *e, const StateView &v, const JobParams &jp, const Since *since, ViewJob *vj) {
  hipStream_t s = e->stream;
  const uint64_t K = v.K, P = v.P;
  DevCounters *ctr = static_cast<DevCounters *>(e->counters.p);
  unsigned long long *tmin_dev = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->counters.p) + kTailHistLen);
  HistBatch &hist = vj->hist;
  int rc;
  vj->off = v.soff;   // EWMA with every point: the row offsets are the series offsets
  if (P == 0) return TAD_OK;
  ViewRoute route;
  if ((rc = carve_buf(e, e->hs_kcnt, &route, view_route_layout, K)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K > P ? K : P) * sizeof(unsigned long long))) != TAD_OK) return rc;
  vj->list = route.list;
  vj->lcount = route.lcount;
  vj->coop_min = win_coop_min(K, P);
  launch_win_route(s, K, v.soff, v.st, vj->coop_min, vj->list, vj->lcount, tmin_dev);
  if (jp.algo != TAD_ALGO_DROP) launch_moments(s, K, v.mom.n, v.mom.avg, v.mom.m2, dev_moments(e), ctr);   // (and n_keys / n_points)
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  if (since) {
    const SinceKeys &sk = since->keys;
    // EWMA's anomalous rows need first[k] alone: the walk counts them itself, so no suffix length is written and nothing is scanned
    const bool first_only = jp.algo == TAD_ALGO_EWMA && !jp.all_points;
    const bool ewma_all = jp.algo == TAD_ALGO_EWMA && jp.all_points;
    launch_win_since(s, K, v.soff, v.st, since->key_since, since->since_t, sk, !first_only, jp.algo == TAD_ALGO_DROP ? &ctr->n_keys : nullptr,
                     since->bucket_s, since->bucket_origin);
    if (!first_only) launch_scan(s, sk.cnt, sk.poff, K, scratch, ewma_all ? dev_total(e) : nullptr);   // (EWMA with every point: the row total)
    vj->first = sk.first;
    if (ewma_all) { vj->off = sk.poff; return TAD_OK; }
  }
  if (jp.algo == TAD_ALGO_EWMA) {
    if (jp.all_points) return TAD_OK;
    launch_win_ewma(s, K, v.soff, v.sval, v.st, v.mom, jp.alpha, vj->coop_min, vj->list, vj->lcount, false, false, static_cast<uint32_t *>(e->n_anom.p), nullptr,
                    OutRows{}, 0, 0, 0, vj->first);
    launch_scan(s, static_cast<const uint32_t *>(e->n_anom.p), static_cast<unsigned long long *>(e->off.p), K,
                static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
    vj->off = static_cast<const unsigned long long *>(e->off.p);
    return TAD_OK;
  }
  if (since) {   // the reported suffixes packed: the batch of new points
    const SinceKeys &sk = since->keys;
    launch_scan(s, sk.chunks, sk.coff, K, scratch);
    unsigned long long reported = 0;
    HIP_TRY(e, hipMemcpyAsync(&reported, sk.poff + K, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipGetLastError());
    vj->syncs = 1;
    SincePts sp;
    if ((rc = carve_buf(e, e->sn_pts, &sp, since_pts_layout, reported ? reported : 1)) != TAD_OK) return rc;
    launch_win_suffix(s, K, reported, v.soff, v.sval, v.st, sk, sp);
    hist.nk = sp.nk; hist.nv = sp.nv; hist.nt = sp.nt; hist.poff = sk.poff; hist.P_dev = sk.poff + K; hist.P_cap = reported;
    if (jp.algo == TAD_ALGO_DBSCAN) return hist_verdicts(e, v.hoff, v.hval, jp, &hist);
    if (jp.algo == TAD_ALGO_DROP) return state_drop_batch(e, v, hist, jp, true, vj->coop_min, vj->list, vj->lcount, ctr, &vj->db);
    return stream_arima_batch(e, v, hist, jp, ctr, &vj->ab);
  }
  if ((rc = ensure(e, e->hs_key, P * 8)) != TAD_OK) return rc;
  unsigned long long *nk = static_cast<unsigned long long *>(e->hs_key.p);
  launch_win_keys(s, K, v.soff, nk);
  hist.nk = nk; hist.nv = v.sval; hist.nt = v.st; hist.poff = v.soff; hist.P_dev = v.soff + K; hist.P_cap = P;
  if (jp.algo == TAD_ALGO_DBSCAN) return hist_verdicts(e, v.hoff, v.hval, jp, &hist);
  if (jp.algo == TAD_ALGO_DROP) return state_drop_batch(e, v, hist, jp, false, vj->coop_min, vj->list, vj->lcount, ctr, &vj->db);
  return stream_arima_batch(e, v, hist, jp, ctr, &vj->ab);
}

// After the round trip (c: the job's counters as the host read them): the result, the emit, the stats.  view_syncs: the host
// synchronisations the caller spent on building the view (tad_stats.host_syncs).  raw_points: the state's points behind a bucketed view
// (tad_stats.rows_in / rows_used); 0: the view's own
int view_rows(JobCtx *e, const StateView &v, const tad_job *job, const JobParams &jp, const ViewJob &vj, const DevCounters &c, uint64_t rows,
              tad_mem out_memory, tad_result **out, int view_syncs, uint64_t raw_points) {
  hipStream_t s = e->stream;
  const uint64_t P = v.P;
  RowsOut ro;
  int rc;
  if ((rc = make_result(e, rows, jp.all_points, out_memory, &ro.rp, &ro.dev_rows, &ro.dev_block)) != TAD_OK) return rc;
  if (rows && jp.algo == TAD_ALGO_EWMA)
    launch_win_ewma(s, v.K, v.soff, v.sval, v.st, v.mom, jp.alpha, vj.coop_min, vj.list, vj.lcount, true, jp.all_points, nullptr, vj.off, ro.dev_rows, rows,
                    e->plan.ewma_emit, e->plan.ewma_emit_rows, vj.first);
  else if (rows)
    emit_point_rows(s, jp, vj.hist, vj.ab, vj.db, v.mom, ro.dev_rows);
  if ((rc = finish_rows(e, job, &ro, rows, jp.all_points, c, P != 0)) != TAD_OK) return rc;
  tad_stats &rs = ro.rp->pub.stats;
  rs.n_points = P;
  rs.rows_in = rs.rows_used = raw_points ? raw_points : P;
  {
    unsigned long long tmin = ~0ull;
    memcpy(&tmin, e->tail_host + kTailHistLen, 8);
    rs.t0 = (P && tmin != ~0ull) ? (int64_t)(tmin ^ (1ull << 63)) : 0;
  }
  hipEventElapsedTime(&rs.ms_total, e->ev[0], e->ev[4]);
  rs.ms_detect = rs.ms_total;   // no Stage 0 ran: the whole call is the detector and its emit
  rs.host_syncs = 2 + view_syncs + vj.syncs;
  e->done.store(4);
  *out = &ro.rp->pub;
  return TAD_OK;
}

// The job on a view after run_view_begin (tad.h; kernels: tad_window.hip): the detector, the one host round trip of the job's tail, the
// rows.  Reads the view only: the state's CURRENT copies, or a window's view in this context's workspace (wv_key / wv_pts, which nothing
// below resizes).
int run_view_locked(JobCtx *e, const StateView &v, const tad_job *job, tad_mem out_memory, tad_result **out, int view_syncs,
                    const Since *since = nullptr, uint64_t raw_points = 0) {
  const JobParams jp = job_params(job);
  ViewJob vj;
  int rc;
  if ((rc = view_detect(e, v, jp, since, &vj)) != TAD_OK) return rc;
  e->done.store(2);
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, hipGetLastError());
  const uint64_t rows = (jp.algo == TAD_ALGO_EWMA && jp.all_points && !since) ? v.P : (v.P ? *e->total_host : 0);
  const DevCounters c = *e->ctr_host;
  e->done.store(3);
  return view_rows(e, v, job, jp, vj, c, rows, out_memory, out, view_syncs, raw_points);
}

// The view of a window of the state in the context's workspace (kernels: tad_window.hip), after run_view_begin, in two steps:
// window_bounds (every key's bounds, the view's offsets, the window's point total — one host round trip) and window_gather (the view
// itself, which run_view_locked then judges).  Both read the state's CURRENT copies and write workspace only: wv_key and wv_pts hold the
// view; run_view_locked resizes neither.
// 1. every key's bounds; the view's offsets and the chunk offsets; *P = the window's point total.  keep (device, K bytes, or NULL): the
// key selection of tad_run_state_keys / tad_drop_state_keys — a key that is not selected gets an empty window
// — and `since` (device, K entries, or NULL) that of tad_run_state_since: so does a key whose entry is kNoChange
int window_bounds(JobCtx *e, const tad_state *st, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *keep, const long long *since,
                  uint64_t *P) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const StateView whole = series_view(st, st->cur);
  int rc;
  WinKeys w;
  if ((rc = carve_buf(e, e->wv_key, &w, win_keys_layout, K)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K) * sizeof(unsigned long long))) != TAD_OK) return rc;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  launch_win_bounds(s, K, whole.soff, whole.st, (long long)from_t, (long long)to_t, keep_points, keep, w.wbeg, w.wlen, w.ecnt, w.chunks, since);
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
int window_gather(JobCtx *e, const tad_state *st, const tad_job *job, uint64_t P, bool subtract, StateView *v) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  const WinKeys w = carve_at(e->wv_key.p, win_keys_layout, K);   // (as window_bounds placed it)
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  int rc;
  *v = StateView{};
  v->K = K;
  v->P = P;
  if (P != 0) {
    const bool dbscan = job->algo == TAD_ALGO_DBSCAN;
    WinPts wp;
    if ((rc = carve_buf(e, e->wv_pts, &wp, win_pts_layout, P, dbscan)) != TAD_OK) return rc;
    unsigned long long *wval = wp.wval, *wh = wp.wh, *ev = nullptr, *es = nullptr;
    long long *wt = wp.wt;
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

// tad_run_state_buckets, in window_gather's place: the view of the window's points FOLDED into time buckets, built straight from the
// state's arrays through window_bounds' wbeg / wlen — no unbucketed copy of the window is written.  The heads per chunk and their scan
// (bk_key), one more host round trip for the bucket total, the fold into wv_pts, then what a window's view gets: the moments by
// launch_trim_moments (a key with a point cut or folded away is replayed over its buckets, a key left whole with every point in a bucket
// of its own keeps the state's) and DBSCAN's history by sorting the buckets' values.  P: the window's points (0: an empty view)
int window_buckets(JobCtx *e, const tad_state *st, const tad_job *job, int64_t bucket_s, int64_t origin, bool op_max, uint64_t P, StateView *v) {
  hipStream_t s = e->stream;
  const uint64_t K = st->K;
  const StateView whole = series_view(st, st->cur);
  const WinKeys w = carve_at(e->wv_key.p, win_keys_layout, K);   // (as window_bounds placed it)
  int rc;
  *v = StateView{};
  v->K = K;
  if (P != 0) {
    const uint64_t bound = trim_chunks_bound(K, whole.P);
    BucketKeys b;
    if ((rc = carve_buf(e, e->bk_key, &b, bucket_keys_layout, K, bound)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(bound > K ? bound : K) * sizeof(unsigned long long))) != TAD_OK) return rc;
    unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
    const BucketSource src{whole.soff, whole.sval, whole.st, w.wbeg, w.wlen};
    launch_win_bucket_heads(s, bound, w.coff, K, src, (long long)bucket_s, (long long)origin, b.hcnt);
    launch_scan(s, b.hcnt, b.hoff, bound, scratch);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemcpyAsync(e->tail_host + kTailTotal, b.hoff + bound, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const uint64_t B = *e->total_host;   // the buckets: at least one per key with a window point, at most P
    const bool dbscan = job->algo == TAD_ALGO_DBSCAN;
    const size_t need = carved_bytes(win_pts_layout, B, dbscan) + carved_bytes(bucket_keys_layout, K, bound) + carved_bytes(win_keys_layout, K);
    if (need > e->ws_limit)   // (the state is only ever read: nothing to undo)
      return fail(e, TAD_ERR_GRID_TOO_LARGE, "tad_run_state_buckets: the view of %llu buckets needs %llu bytes > workspace limit %llu (state unchanged)",
                  (unsigned long long)B, (unsigned long long)need, (unsigned long long)e->ws_limit);
    WinPts bp;
    if ((rc = carve_buf(e, e->wv_pts, &bp, win_pts_layout, B, dbscan)) != TAD_OK) return rc;
    launch_win_bucket_fold(s, bound, w.coff, K, src, (long long)bucket_s, (long long)origin, op_max, b.hoff, B, bp.wval, bp.wt);
    launch_win_bucket_keys(s, K, whole.soff, w.coff, b.hoff, b.boff, b.bcnt, b.becnt);
    const double alpha = job->ewma_alpha == 0.0 ? 0.5 : job->ewma_alpha;   // (for the view's ewma only, which no detector reads)
    launch_trim_moments(s, K, b.bcnt, b.becnt, b.boff, bp.wval, alpha, whole.mom, w.wmom);
    if (dbscan) launch_hist_sort(s, bp.wval, b.boff, K, bp.wh, w.chunks, w.long_count);   // (chunks: read for the last time by the scan to coff)
    HIP_TRY(e, hipGetLastError());
    v->P = B;
    v->soff = b.boff; v->sval = bp.wval; v->st = bp.wt; v->mom = w.wmom;
    if (dbscan) { v->hoff = b.boff; v->hval = bp.wh; }
  }
  e->done.store(1);
  return TAD_OK;
}

// What the five calls refuse before they take the state's lock.  Both families check the same things in the same order; the family
// supplies the algorithm test with its message, the parameter ranges and DBSCAN's history.  who: the call's name in the messages; narrow:
// where the caller narrows the window instead of start_time / end_time.
enum class Family { Run, Drop };   // Run: EWMA, DBSCAN, ARIMA; Drop: DROP

int check_view_job(tad_engine *eng, const tad_state *st, const tad_job *job, tad_result **out, const char *who, Family family, const char *narrow) {
  const bool drop = family == Family::Drop;
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "%s: engine is NULL", who);
  if (!st || !job || !out) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: state, job and out must not be NULL", who);
  *out = nullptr;
  if (drop && job->algo != TAD_ALGO_DROP)   // (the message names the Run call with the same arguments)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be DROP (%s judges EWMA, DBSCAN and ARIMA)", who,
                strstr(who, "_keys") ? "tad_run_state_keys" : "tad_run_state_window");
  if (!drop && job->algo != TAD_ALGO_EWMA && job->algo != TAD_ALGO_DBSCAN && job->algo != TAD_ALGO_ARIMA)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the algorithm must be EWMA, DBSCAN or ARIMA (DROP: tad_drop_state)", who);
  if (job->start_time != 0 || job->end_time != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: start_time / end_time must be 0: %s", who, narrow);
  if (job->flags & (TAD_FLAG_KEY_U32 | TAD_FLAG_TIME_U32))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32 describe input columns; there are none", who);
  if (drop ? (!(job->drop_nsigma >= 0.0) || job->drop_min_samples < 0)
           : (job->ewma_alpha < 0.0 || job->ewma_alpha > 1.0 || job->dbscan_eps < 0.0 || job->dbscan_min_samples < 0 || job->arima_maxiter < 0))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: detector parameter out of range", who);
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state must keep its series with times (TAD_STATE_SERIES | TAD_STATE_TIMES)", who);
  if (job->algo == TAD_ALGO_DBSCAN && !st->history)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: DBSCAN needs a state with history too (TAD_STATE_HISTORY)", who);
  return TAD_OK;
}

// Which of the state's points a call judges: of every key's series the points with from_t <= flow_end_s < to_t (0 = no bound on that
// side), of those the newest keep_points (0 = all), and only of the keys whose byte in key_keep is not 0 (NULL, length 0 = every key).
// All zero is the whole state.
struct Window {
  int64_t from_t = 0, to_t = 0;
  uint64_t keep_points = 0;
  const uint8_t *key_keep = nullptr;
  uint64_t key_keep_len = 0;
  tad_mem key_memory = TAD_MEM_HOST;
  // tad_run_state_since / tad_drop_state_since: of the judged points, the ones that are reported (key_since: key_keep_len entries, in
  // key_memory; an entry of TAD_NO_CHANGE also takes the key out of the selection)
  const int64_t *key_since = nullptr;
  int64_t since_t = 0;
  // tad_run_state_buckets: the judged points folded into time buckets of bucket_s seconds (0: judged as they are, the other calls)
  int64_t bucket_s = 0, bucket_origin = 0;
  bool bucket_max = false;
};

const char *const kNarrowWindow = "the window is from_t / to_t / keep_points";

// The checked job (check_view_job) over the window w of the state, under the name who.  A key whose byte is 0 is left empty by
// window_bounds, and the rest of the call treats it as any key the window left empty.  The mask is a window of its own, so with one the
// "no window at all" shortcut is not taken; P == S still is, since then every point the state holds is selected.  DROP: values and times
// only, no moments, no history.
int view_call(tad_engine *eng, tad_state *st, const tad_job *job, const char *who, const Window &w, tad_mem out_memory, tad_result **out) {
  if (w.from_t != 0 && w.to_t != 0 && w.from_t > w.to_t) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: from_t is later than to_t", who);
  if (!w.key_keep && !w.key_since && w.key_keep_len != 0)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep is NULL with a length of %llu", who, (unsigned long long)w.key_keep_len);
  if ((w.key_keep || w.key_since) && w.key_memory != TAD_MEM_HOST && w.key_memory != TAD_MEM_DEVICE)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: %s must be in host or device memory", who,
                w.key_keep && w.key_since ? "key_keep and key_since" : (w.key_since ? "key_since" : "key_keep"));
  if (reinterpret_cast<uintptr_t>(w.key_since) % 8 != 0) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_since must be 8-byte aligned", who);
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times)", who);
  if (w.key_keep && w.key_keep_len != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_keep has %llu entries, the state holds %llu keys", who, (unsigned long long)w.key_keep_len,
                (unsigned long long)st->K);
  if (w.key_since && w.key_keep_len != st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: key_since has %llu entries, the state holds %llu keys", who, (unsigned long long)w.key_keep_len,
                (unsigned long long)st->K);
  int rc;
  if ((rc = call.enter(who, job->id, job->algo == TAD_ALGO_ARIMA)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  if ((rc = run_view_begin(e, st->K)) != TAD_OK) return rc;
  const StateView whole = series_view(st, st->cur);
  const uint64_t S = whole.P;
  // with no since at all the call is the *_keys call: `since` stays NULL and nothing below differs
  Since since_args;
  const Since *since = nullptr;
  if (w.key_since || w.since_t != 0) {
    const bool staged = w.key_since && w.key_memory == TAD_MEM_HOST;
    if ((rc = carve_buf(e, e->sn_key, &since_args.keys, since_keys_layout, st->K, staged)) != TAD_OK) return rc;
    since_args.since_t = (long long)w.since_t;
    since_args.key_since = reinterpret_cast<const long long *>(w.key_since);
    if (staged && st->K != 0) {
      HIP_TRY(e, hipMemcpyAsync(since_args.keys.since, w.key_since, (size_t)st->K * 8, hipMemcpyHostToDevice, e->stream));
      since_args.key_since = since_args.keys.since;
    }
    since_args.bucket_s = (long long)w.bucket_s;
    since_args.bucket_origin = (long long)w.bucket_origin;
    since = &since_args;
  }
  const long long *d_since = since ? since->key_since : nullptr;
  const bool bucketed = w.bucket_s != 0;   // (then neither shortcut below is taken: a whole key is still folded)
  if (S == 0 || (!bucketed && !w.key_keep && !d_since && w.from_t == 0 && w.to_t == 0 && w.keep_points == 0))
    return run_view_locked(e, whole, job, out_memory, out, 0, since);
  const uint8_t *d_keep = w.key_keep;
  if (w.key_keep && w.key_memory == TAD_MEM_HOST) {   // staged: only window_bounds reads it
    if ((rc = ensure(e, e->in_key, (size_t)st->K)) != TAD_OK) return rc;
    HIP_TRY(e, hipMemcpyAsync(e->in_key.p, w.key_keep, st->K, hipMemcpyHostToDevice, e->stream));
    d_keep = static_cast<const uint8_t *>(e->in_key.p);
  }
  uint64_t P = 0;
  if ((rc = window_bounds(e, st, w.from_t, w.to_t, w.keep_points, d_keep, d_since, &P)) != TAD_OK) return rc;
  if (bucketed) {
    StateView v;
    if ((rc = window_buckets(e, st, job, w.bucket_s, w.bucket_origin, w.bucket_max, P, &v)) != TAD_OK) return rc;
    return run_view_locked(e, v, job, out_memory, out, P ? 2 : 1, since, P);
  }
  if (P == S) return run_view_locked(e, whole, job, out_memory, out, 1, since);   // every key is selected and whole: the state's own arrays, no view
  const bool subtract = job->algo == TAD_ALGO_DBSCAN && P != 0 && !win_hist_by_sort(P, S);   // (P: the SELECTED window points)
  StateView v;
  if ((rc = window_gather(e, st, job, P, subtract, &v)) != TAD_OK) return rc;
  return run_view_locked(e, v, job, out_memory, out, 1, since);
}

// tad_run_state_since / tad_drop_state_since: the report window's own checks, then the call
int since_call(tad_engine *eng, tad_state *st, const tad_job *job, const char *who, Family family, const tad_report_window *w, tad_mem out_memory,
               tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, who, family, "the window is the report window's from_t / to_t / keep_points");
  if (rc != TAD_OK) return rc;
  if (!w) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the report window must not be NULL", who);
  Window win{w->from_t, w->to_t, w->keep_points, w->key_keep, (w->key_keep || w->key_since) ? w->num_keys : 0, w->key_memory};
  win.key_since = w->key_since;
  win.since_t = w->since_t;
  return view_call(eng, st, job, who, win, out_memory, out);
}

}  // namespace

extern "C" {

// the rule view_call decides DBSCAN's history with
int tad_window_history_by_sort(uint64_t window_points, uint64_t state_points) { return win_hist_by_sort(window_points, state_points) ? 1 : 0; }

int tad_run_state(tad_engine *eng, tad_state *st, const tad_job *job, tad_mem out_memory, tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, "tad_run_state", Family::Run, "the window is what the state holds (tad_state_trim narrows it)");
  return rc != TAD_OK ? rc : view_call(eng, st, job, "tad_run_state", Window{}, out_memory, out);
}

int tad_run_state_window(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, tad_mem out_memory,
                         tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, "tad_run_state_window", Family::Run, kNarrowWindow);
  return rc != TAD_OK ? rc : view_call(eng, st, job, "tad_run_state_window", Window{from_t, to_t, keep_points}, out_memory, out);
}

int tad_drop_state(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, tad_mem out_memory,
                   tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, "tad_drop_state", Family::Drop, kNarrowWindow);
  return rc != TAD_OK ? rc : view_call(eng, st, job, "tad_drop_state", Window{from_t, to_t, keep_points}, out_memory, out);
}

int tad_run_state_keys(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *key_keep,
                       uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, "tad_run_state_keys", Family::Run, kNarrowWindow);
  return rc != TAD_OK ? rc : view_call(eng, st, job, "tad_run_state_keys", Window{from_t, to_t, keep_points, key_keep, key_keep_len, key_memory}, out_memory, out);
}

int tad_drop_state_keys(tad_engine *eng, tad_state *st, const tad_job *job, int64_t from_t, int64_t to_t, uint64_t keep_points, const uint8_t *key_keep,
                        uint64_t key_keep_len, tad_mem key_memory, tad_mem out_memory, tad_result **out) {
  const int rc = check_view_job(eng, st, job, out, "tad_drop_state_keys", Family::Drop, kNarrowWindow);
  return rc != TAD_OK ? rc : view_call(eng, st, job, "tad_drop_state_keys", Window{from_t, to_t, keep_points, key_keep, key_keep_len, key_memory}, out_memory, out);
}

int tad_run_state_since(tad_engine *eng, tad_state *st, const tad_job *job, const tad_report_window *w, tad_mem out_memory, tad_result **out) {
  return since_call(eng, st, job, "tad_run_state_since", Family::Run, w, out_memory, out);
}

int tad_drop_state_since(tad_engine *eng, tad_state *st, const tad_job *job, const tad_report_window *w, tad_mem out_memory, tad_result **out) {
  return since_call(eng, st, job, "tad_drop_state_since", Family::Drop, w, out_memory, out);
}

// the since call with three more fields of the one window: the bucket window's own checks, then the call
int tad_run_state_buckets(tad_engine *eng, tad_state *st, const tad_job *job, const tad_bucket_window *w, tad_mem out_memory, tad_result **out) {
  const char *who = "tad_run_state_buckets";
  const int rc = check_view_job(eng, st, job, out, who, Family::Run, "the window is the bucket window's from_t / to_t / keep_points");
  if (rc != TAD_OK) return rc;
  if (!w) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the bucket window must not be NULL", who);
  if (!bucket_args_ok(w->bucket_s, w->bucket_origin))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bucket_s must be >= 1 and 0 <= bucket_origin < bucket_s (got %lld, %lld)", who, (long long)w->bucket_s,
                (long long)w->bucket_origin);
  if (w->bucket_op != TAD_OP_SUM && w->bucket_op != TAD_OP_MAX)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bucket_op must be TAD_OP_SUM or TAD_OP_MAX", who);
  Window win{w->from_t, w->to_t, w->keep_points, w->key_keep, (w->key_keep || w->key_since) ? w->num_keys : 0, w->key_memory};
  win.key_since = w->key_since;
  win.since_t = w->since_t;
  win.bucket_s = w->bucket_s;
  win.bucket_origin = w->bucket_origin;
  win.bucket_max = w->bucket_op == TAD_OP_MAX;
  return view_call(eng, st, job, who, win, out_memory, out);
}

}  // extern "C"
