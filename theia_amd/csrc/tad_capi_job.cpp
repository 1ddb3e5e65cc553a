// tad_capi_job.cpp — the batch job of include/tad.h: tad_run / tad_aggregate / tad_run_stream, and the Stage 0 that tad_drop_stream and
// tad_state_merge run through (tad_capi.cpp; the read-only jobs on a state, which run no Stage 0, are tad_capi_view.cpp).  Replaces one run of anomaly_detection() (plugins/anomaly-detection/anomaly_detection.py:647-710):
// Stage 0 GROUP BY -> per-key sigma -> detector -> compaction.  run_job_locked reads as the sequence of its stages: the lattice, Stage 0
// (sparse, tiles or scatter), the count pass, the retry rules' word (tad_stage0_retry.h), the result.
#include "tad_engine.h"

using namespace tad;
using namespace tadh;

namespace {

// What one job brings to each of its attempts.
struct Job {
  const tad_job *job;
  const tad_columns *cols;
  tad_state *stream;           // one streaming batch
  bool points_mode;            // Stage 0 alone (tad_aggregate)
  int depth;                   // > 0: a length class of a skewed sparse table run as a job of its own
  tad_mem out_memory;
  JobParams jp;
  tad_plan plan;               // the engine's plan when the job was admitted
  bool op_max, has2;
  uint64_t K, slots_all;
  RowFilter rf;
  RowCols rows;                // the table on the device (stage_columns).  rows.cw: narrow input columns (tad.h, tad_columns) are read at their own
                               // width by the Stage-0 kernels, nothing is widened first
  DevCounters *ctr;
  bool empty;                  // no live row: nothing to group
};

// What the stages of one attempt hand on.
struct Attempt {
  bool retry = false;      // the retry rules have advanced: run the attempt again
  bool finished = false;   // the job has returned its result from inside a stage (length classes, Stage 0 alone on the sorted list)
  bool hinted = false;     // the lattice is the caller's
  PartPlan pl{};
  Lattice L{};
  Grid g{};
  uint64_t cells = 0, need = 0;
  bool cells_overflow = false;
  bool v2 = false, sparse = false, sp_part = false, hist_sampled = false, use_kh = false, narrow_tiles = false;
  const uint32_t *binhist = nullptr;
  const unsigned long long *stream_poff = nullptr;   // a sparse streaming batch: key k's points at [poff[k], poff[k + 1]) of the sorted list
  uint64_t stream_P = 0;                             // ... and the number of its points
  int stage0_path() const { return sparse ? (sp_part ? 8 : 4) : (v2 ? (pl.wc_cap ? 3 : 2) : 1); }
  int hist_source() const { return (v2 && hist_sampled) ? 1 : (use_kh ? 2 : 0); }   // tad_stats.hist_sampled
};

// Asks the retry rules what the attempt's facts so far mean: TAD_OK with a.retry clear (go on) or set (run the attempt again), or the
// job's error.
int decide(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a, Stage0Facts f) {
  f.v2 = a.v2; f.sparse = a.sparse; f.sp_part = a.sp_part; f.use_kh = a.use_kh; f.hist_sampled = a.hist_sampled; f.narrow_tiles = a.narrow_tiles;
  const Stage0Next x = rs.next(f);
  a.retry = x.what == Stage0Next::kRetry;
  if (x.what != Stage0Next::kFail) return TAD_OK;
  if (x.code == TAD_ERR_GRID_TOO_LARGE)
    return fail(e, x.code, x.msg, (unsigned long long)a.need, (unsigned long long)j.K, (unsigned long long)a.L.nb, (long long)a.L.step, (unsigned long long)e->ws_limit);
  return fail(e, x.code, x.msg, (unsigned long long)j.K);
}

int decide(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a, uint32_t err) {
  Stage0Facts f;
  f.err = err;
  return decide(e, j, rs, a, f);
}

int detect_and_count(JobCtx *e, Grid g, JobParams &jp, DevCounters *ctr, uint64_t *rows) {
  hipStream_t s = e->stream;
  int rc;
  if ((rc = ensure_key_buffers(e, g.K)) != TAD_OK) return rc;
  if ((rc = ensure_rcp_table(e, g.T)) != TAD_OK) return rc;
  double *sigma = static_cast<double *>(e->sigma.p);
  uint32_t *n_pts = static_cast<uint32_t *>(e->n_pts.p);
  uint32_t *n_anom = static_cast<uint32_t *>(e->n_anom.p);
  unsigned long long *off = static_cast<unsigned long long *>(e->off.p);

  const bool ewma = jp.algo == TAD_ALGO_EWMA;
  const bool drop = jp.algo == TAD_ALGO_DROP;
  // DBSCAN ignores sigma for its verdicts (anomaly_detection.py:325-349) — it is only an output column of the anomalous
  // rows.  The tile kernel then delivers the per-key counts / moments itself and k_emit streams stddev_samp for the keys
  // that have rows: no separate per-key walk over the whole grid (C4: -0.44 ms).  emit-all jobs keep the general path.
  const bool db_fused = jp.algo == TAD_ALGO_DBSCAN && !jp.all_points && dbscan_uses_list(g);
  jp.lazy_sigma = db_fused;
  if (drop) {   // mean / std / verdicts / counters in one kernel (pandas' pairwise arithmetic, not Spark's streaming update)
    if ((rc = ensure(e, e->calc, (g.K * g.T ? g.K * g.T : 1) * sizeof(double))) != TAD_OK) return rc;
    launch_drop(s, g, jp.drop_nsigma, jp.drop_min_samples, static_cast<double *>(e->calc.p), sigma, n_pts,
                static_cast<double *>(e->key_mean.p), static_cast<double *>(e->key_m2.p), ctr);
  } else if (!db_fused)
    launch_key_sigma(s, g, jp.alpha, ewma && !jp.all_points, static_cast<const double *>(e->rcp_table.p), sigma, n_pts, n_anom, ctr, static_cast<double *>(e->key_mean.p),
                     static_cast<double *>(e->key_m2.p));
  if (jp.algo == TAD_ALGO_DBSCAN) {
    if ((rc = ensure(e, e->aux, dbscan_scratch_bytes(g))) != TAD_OK) return rc;
    if (dbscan_uses_list(g)) {
      DbscanStats dst{nullptr, nullptr, nullptr, nullptr};
      if (db_fused) dst = DbscanStats{n_pts, n_anom, static_cast<double *>(e->key_mean.p), static_cast<double *>(e->key_m2.p)};
      if (launch_dbscan(s, g, jp.eps, jp.min_samples, e->aux.p, dst, jp.settled && db_fused) != 0)
        return fail(e, TAD_ERR_HIP, "DBSCAN launch failed");
    } else {
      return fail(e, TAD_ERR_GRID_TOO_LARGE, "DBSCAN: series of %llu buckets are not supported", (unsigned long long)g.T);
    }
  } else if (jp.algo == TAD_ALGO_ARIMA) {
    if ((rc = ensure(e, e->calc, g.K * g.T * sizeof(double))) != TAD_OK) return rc;
    const size_t wsb = arima_workspace_bytes(g);
    if ((rc = ensure(e, e->aux, wsb)) != TAD_OK) return rc;
    // The fit yields to whole-CU jobs of other contexts (arima_yield_loop).  This job's own claim is dropped for the duration (it would pause
    // itself) and taken back for the emit.
    const bool held = e->hold && e->hold->held;
    if (held) e->hold->release();
    const unsigned int *yielded_dev = nullptr;
    if (launch_arima(s, g, sigma, n_pts, jp.maxiter, static_cast<double *>(e->calc.p), ctr, e->aux.p, wsb, e->eng->pause_dev, &yielded_dev) != 0)
      return fail(e, TAD_ERR_HIP, "ARIMA launch failed");
    if ((rc = arima_yield_loop(e, yielded_dev, [&](uint32_t grace, const unsigned int **yd) {
           return launch_arima_fit(s, g, sigma, n_pts, jp.maxiter, static_cast<double *>(e->calc.p), ctr, e->aux.p, e->eng->pause_dev, yd, grace);
         })) != TAD_OK)
      return rc;
    if (held) e->hold->acquire();
  }
  const uint32_t *cnt = n_anom;
  if (jp.all_points && jp.algo != TAD_ALGO_ARIMA && !drop) cnt = n_pts;
  else if (db_fused) {}                                                             // the tile kernel counted the noise points
  else if (!ewma || jp.all_points) launch_count_flags(s, g, jp.all_points, n_anom);  // ARIMA / DROP all_points: skips no-result keys
  launch_scan_moments(s, cnt, off, g.K, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e), n_pts,
                      static_cast<const double *>(e->key_mean.p), static_cast<const double *>(e->key_m2.p), dev_moments(e), db_fused ? ctr : nullptr);
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  *rows = *e->total_host;
  return TAD_OK;
}

// width: bytes per row of the column (8, or 4 for a narrow key / time column): a host column crosses PCIe at its own width
template <typename T>
int stage_column(JobCtx *e, DevBuf &buf, const T *src, uint64_t n, tad_mem mem, const T **dev, uint64_t width = 8) {
  if (!src) { *dev = nullptr; return TAD_OK; }
  if (mem == TAD_MEM_DEVICE) { *dev = src; return TAD_OK; }
  int rc = ensure(e, buf, n * width);
  if (rc != TAD_OK) return rc;
  HIP_TRY(e, hipMemcpyAsync(buf.p, src, n * width, hipMemcpyHostToDevice, e->stream));
  *dev = static_cast<const T *>(buf.p);
  return TAD_OK;
}

int stage_columns(JobCtx *e, Job &j) {
  const tad_columns *cols = j.cols;
  RowCols &r = j.rows;
  const uint64_t kw = (r.cw & kColKey32) ? 4 : 8, tw = (r.cw & kColTime32) ? 4 : 8;
  int rc;
  if ((rc = stage_column(e, e->in_key, cols->key_id, r.n, cols->memory, &r.key, kw)) != TAD_OK) return rc;
  if ((rc = stage_column(e, e->in_key2, cols->key_id2, r.n, cols->memory, &r.key2, kw)) != TAD_OK) return rc;
  if ((rc = stage_column(e, e->in_te, cols->flow_end_s, r.n, cols->memory, &r.t_end, tw)) != TAD_OK) return rc;
  if ((rc = stage_column(e, e->in_ts, cols->flow_start_s, r.n, cols->memory, &r.t_start, tw)) != TAD_OK) return rc;
  return stage_column(e, e->in_val, cols->value, r.n, cols->memory, &r.value);
}

// ---- the time lattice ----

// Pass A of Stage 0 v2: lattice partials + per-workgroup key-bin histogram in one read of the key / time columns.  Decides a.v2, where
// pass B's region sizes come from (a.binhist, a.use_kh, a.hist_sampled), and returns the number of partials it left in e->meta.
int pass_a(JobCtx *e, const Job &j, const Stage0Retry &rs, Attempt &a, int *meta_blocks) {
  hipStream_t s = e->stream;
  int rc;
  const uint64_t n = j.rows.n, K = j.K;
  a.v2 = !j.empty && j.plan.stage0 != 1 && !rs.v1 && (j.plan.stage0 == 2 || n >= (1ull << 22)) && part_plan_bins(n, K, j.has2, &a.pl);
  if (a.v2 && e->hold) e->hold->acquire();   // pass B / pass C workgroups need whole CUs: ARIMA fits of other jobs in flight make room (PauseHold)
  if ((rc = ensure(e, e->meta, sizeof(MetaPartial) * kMetaBlocks)) != TAD_OK) return rc;
  *meta_blocks = 0;
  if (!a.v2) return TAD_OK;
  const PartPlan &pl = a.pl;
  // The caller's key-bin histogram (tad_factorize_hist's by-product): pass A then only samples the time lattice and pass B's regions are
  // sized EXACTLY from the caller's counts.  Taken when it provably describes this batch and this job: same rows, keys, sides and row
  // chunking, no time-window filter (the histogram counted every kept row), the lattice still derived from a sample (lat_mode 1 or a hint).
  const tad_key_hist *kh = j.cols->key_hist;
  a.use_kh = j.depth == 0 && !rs.kh_rejected && kh != nullptr && kh->bins != nullptr && rs.lat_mode != 2 && kh->n_rows == n && kh->num_keys == K &&
             kh->sides == (j.has2 ? 2u : 1u) && kh->workgroups == (uint32_t)pl.G && kh->nbins == pl.nbins && kh->shift == (uint32_t)pl.shift_bin &&
             kh->chunk_rows == pl.chunk && j.rf.end_time == 0 && !(j.rows.t_start != nullptr && j.rf.start_time != 0);
  if ((rc = ensure(e, e->binhist, (size_t)pl.G * pl.nbins * 4)) != TAD_OK) return rc;
  // pass A may histogram a SAMPLE of the rows (1/16 of the key column, plus the chunk ends, instead of all of it): pass B's regions are then
  // sized from the estimate with 6 sigma of slack; a region that still turns out too small (keys arriving in bursts the sample missed)
  // raises DEV_ERR_REGION_FULL and the job is redone with the exact histogram.  tad_plan.histogram = 1 disables it.
  a.hist_sampled = launch_meta_hist(s, j.rows, K, j.rf, pl, static_cast<MetaPartial *>(e->meta.p), static_cast<uint32_t *>(e->binhist.p), j.ctr,
                                    // small regions (many keys: C4 has ~50 records per workgroup and 128-key block) make pass C's walk
                                    // over the regions cost more than the sampled pass A saves: sample only when a region of a
                                    // 128-key block is expected to hold a few hundred records
                                    // (lat_mode 2 re-derives the lattice with k_meta, which reuses the partials buffer the sampling ratios live in)
                                    a.use_kh ||       // (the sampled pass: its histogram lands in e->binhist and is not used)
                                    (!rs.exact_hist && rs.lat_mode != 2 && sampled_slots_bound(j.slots_all, pl) < (1ull << 32) &&
                                        (j.plan.histogram == 2 ||      // (A/B: sampled wherever it is possible at all)
                                         j.slots_all / ((uint64_t)pl.G * ((K >> kSampleBlockShift) ? (K >> kSampleBlockShift) : 1)) >= 384)));
  *meta_blocks = pl.G;
  a.binhist = static_cast<const uint32_t *>(e->binhist.p);
  if (a.use_kh && a.hist_sampled) { a.binhist = kh->bins; a.hist_sampled = false; }   // exact counts, from the caller
  else a.use_kh = false;          // (pass A could not sample — unaligned columns — and counted every row itself)
  return TAD_OK;
}

// The attempt's lattice a.L: the caller's hint, or derived from pass A's sample (v2) / every row (k_meta: v1, or lat_mode 2) with one
// host round trip.  Sets j.empty when the exact pass found no live row.
int derive_lattice(JobCtx *e, Job &j, Stage0Retry &rs, Attempt &a) {
  hipStream_t s = e->stream;
  int rc, meta_blocks = 0;
  a.hinted = rs.lat_mode == 0;
  a.L = make_lattice(j.cols->t0, a.hinted ? j.cols->step : 1, j.cols->n_buckets);
  if ((rc = pass_a(e, j, rs, a, &meta_blocks)) != TAD_OK) return rc;
  if (!a.hinted && !j.empty && (!a.v2 || rs.lat_mode == 2)) {
    meta_blocks = (int)((j.rows.n + 255) / 256);
    if (meta_blocks > kMetaBlocks) meta_blocks = kMetaBlocks;
    launch_meta(s, j.rows, j.rf, static_cast<MetaPartial *>(e->meta.p), meta_blocks);
  }
  if (!a.hinted && !j.empty) {
    HIP_TRY(e, hipMemcpyAsync(e->meta_host, e->meta.p, sizeof(MetaPartial) * meta_blocks, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    int64_t tmin = 0, tmax = 0, tref = 0;
    uint64_t g = 0, used = 0;
    for (int b = 0; b < meta_blocks; ++b) {
      const MetaPartial &p = e->meta_host[b];
      if (p.used == 0) continue;
      if (used == 0) { tmin = p.tmin; tmax = p.tmax; tref = p.tref; g = p.g; }
      else {
        if (p.tmin < tmin) tmin = p.tmin;
        if (p.tmax > tmax) tmax = p.tmax;
        const uint64_t d = p.tref >= tref ? (uint64_t)p.tref - (uint64_t)tref : (uint64_t)tref - (uint64_t)p.tref;
        g = host_gcd(host_gcd(g, p.g), d);
      }
      used += p.used;
    }
    if (used == 0) {
      Stage0Facts f;
      f.sample_no_live_row = true;
      if ((rc = decide(e, j, rs, a, f)) != TAD_OK || a.retry) return rc;
      j.empty = true;
    } else {
      const uint64_t span = (uint64_t)tmax - (uint64_t)tmin;
      // the lattice must contain tmin and tmax whatever the sample saw
      const uint64_t step = host_gcd(host_gcd(g, span), (uint64_t)tref - (uint64_t)tmin);
      a.L = make_lattice(tmin, (int64_t)(step == 0 ? 1 : step), span / (step == 0 ? 1 : step) + 1);
    }
  }
  HIP_TRY(e, hipEventRecord(e->ev[1], s));
  if (j.depth == 0) e->done.store(1);
  if (j.empty) { a.L = make_lattice(0, 1, 0); a.v2 = false; }
  return TAD_OK;
}

// ---- Stage 0: GROUP BY (key, flowEndSeconds) into the time-major point grid ----

// The dense grid's size and whether the table is sparse.  Sparse tables (few points per key on a fine lattice: second-resolution
// timestamps, per-connection keys): the dense K x T grid would be mostly empty or not fit at all — the rows are sorted by (key, time)
// instead and each key's points laid out by rank (tad_sparse.hip).  Chosen when the rows could fill at most 1/8 of a large grid, or the
// grid does not fit.
int choose_stage0(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a) {
  const uint64_t K = j.K;
  a.cells = j.empty ? 0 : K * a.L.nb;
  a.cells_overflow = !j.empty && a.L.nb != 0 && a.cells / a.L.nb != K;
  // (ARIMA: predictions + 60 B per cell of workspace, arima_workspace_bytes; DROP: one double per cell)
  // (a tad_drop_stream batch judges the state's packed series, tad_drop_state.hip: no workspace per cell, the EWMA batch's rule)
  a.need = a.cells * 9 + (j.jp.algo == TAD_ALGO_ARIMA ? a.cells * 80 + (1ull << 22) : (j.jp.algo == TAD_ALGO_DROP && !j.stream ? a.cells * 8 : 0));
  // (first[], len[] and the class offsets are 32-bit indices into the sorted point list: 2^32 slots and beyond stay dense or fail cleanly)
  // (a streaming batch takes the same rule: its dense grid is state keys x batch span, whatever the batch's rows)
  a.sparse = !j.empty && K <= 0xFFFFFFFFull && j.slots_all < (1ull << 32) &&
             (j.plan.sparse == 2 ||
              (j.plan.sparse != 1 && (a.cells_overflow || a.need > e->ws_limit || (a.cells >= (1ull << 24) && j.slots_all < a.cells / 8))));
  return decide(e, j, rs, a, 0u);   // (a sparse table with the caller's histogram: the job counts for itself)
}

// the sparse Stage 0's sort: its buffers and what the one round trip brought
struct SparseSort {
  PartPlan spl{};
  size_t tb = 0;                               // bytes of sort workspace in e->sp_temp, d_runs behind them
  unsigned long long *d_runs = nullptr;        // [0] runs, [1] tmax
  unsigned long long *ucomp = nullptr, *uval = nullptr;   // e->sp_comp_a / e->sp_val_a: the sorted unique points
  uint64_t P = 0;                              // points (the filtered-out slots sort last and the reduction drops them)
  unsigned int tmax = 0;                       // the longest series
};

// first[] / the longest series from the device-resident point count
void sparse_first_tmax(JobCtx *e, const Job &j, const SparseSort &ss) {
  launch_sparse_tmax(e->stream, ss.ucomp, j.slots_all, ss.d_runs, static_cast<uint32_t *>(e->sp_first.p), reinterpret_cast<unsigned int *>(ss.d_runs + 1));
}

// the partition sort leaves its points in the stages: the sorted list is only built for those who read it
void sparse_sorted_list(JobCtx *e, const Job &j, const Attempt &a, const SparseSort &ss) {
  if (!a.sp_part) return;
  launch_sparse_compact(e->stream, ss.spl, e->sp_temp.p, static_cast<const unsigned long long *>(e->sp_comp_b.p), static_cast<const unsigned long long *>(e->sp_val_b.p),
                        ss.ucomp, ss.uval);
  sparse_first_tmax(e, j, ss);
}

// The rows sorted by (key, time) and reduced to unique points: through the partition pass + LDS sort (a.sp_part) or the LSD radix sort;
// then ONE round trip for the point count and the longest series (and the partition sort's error word, which the retry rules read).
int sparse_sort(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a, SparseSort &ss) {
  hipStream_t s = e->stream;
  int rc;
  const uint64_t n = j.rows.n, K = j.K, slots_all = j.slots_all;
  const Lattice L = a.L;
  // Big sparse tables (pass A ran with its key-bin histogram): the dense path's partition pass brings every key block's rows together as
  // 8-byte records, a workgroup per key sub-range sorts them in LDS (tad_sparse.hip: launch_sparse_sort) — the columns are read once and
  // the records move through HBM once, where the LSD sort moves 16-byte pairs once per digit.  Needs the exact histogram.
  PartPlan &spl = ss.spl;
  spl = a.pl;
  a.sp_part = a.v2 && !rs.sparse_lsd && part_plan_sparse(K, L.nb, j.has2, &spl);
  if (a.sp_part) {
    part_plan_wc(slots_all, j.rows.aligned16(), j.has2, 2, &spl);
    if (spl.wc_cap == 0 || slots_all + spl.pad_slots >= (1ull << 32)) a.sp_part = false;
  }
  if ((rc = decide(e, j, rs, a, 0u)) != TAD_OK || a.retry) return rc;   // (the partition sort after a sampled pass A: the exact histogram first)
  a.v2 = false;
  // (the partition sort: comp_a = the records by round, val_a = the staged ranks until the sorted list — if anyone needs it — takes their place;
  //  the b buffers = the staged points; a round's place is its block's record offset, fillers of pass B included)
  const uint64_t stage_slots = slots_all + (a.sp_part ? spl.pad_slots : 0);
  if ((rc = ensure(e, e->sp_comp_a, stage_slots * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->sp_comp_b, stage_slots * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->sp_val_a, stage_slots * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->sp_val_b, stage_slots * 8)) != TAD_OK) return rc;
  size_t tb = sparse_sort_temp_bytes(slots_all);
  if (a.sp_part && sparse_part_temp_bytes(spl) > tb) tb = sparse_part_temp_bytes(spl);
  if ((uint64_t)slots_all * 32 + tb > e->ws_limit)   // the four sort buffers count against the workspace too: fail cleanly, not in hipMalloc
    return fail(e, TAD_ERR_GRID_TOO_LARGE, "sparse Stage 0 needs %llu bytes of sort buffers for %llu row slots > workspace limit %llu",
                (unsigned long long)(slots_all * 32 + tb), (unsigned long long)slots_all, (unsigned long long)e->ws_limit);
  SparseTemp temp;
  if ((rc = carve_buf(e, e->sp_temp, &temp, sparse_temp_layout, tb)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->sp_first, K * 4 + 64)) != TAD_OK) return rc;
  ss.tb = tb;
  ss.d_runs = temp.runs;
  HIP_TRY(e, hipMemsetAsync(ss.d_runs, 0, 16, s));
  HIP_TRY(e, hipEventRecord(e->ev[2], s));
  unsigned long long *ucomp = ss.ucomp = static_cast<unsigned long long *>(e->sp_comp_a.p), *uval = ss.uval = static_cast<unsigned long long *>(e->sp_val_a.p);
  // (the sort covers bit_width(span) time bits: a row beyond the lattice's last bucket raises DEV_ERR_OFF_LATTICE like a row before t0)
  const uint64_t span = L.nb ? (L.nb - 1) * (uint64_t)L.step : 0;
  if (a.sp_part) {
    const uint64_t slots = slots_all + spl.pad_slots;
    if ((rc = ensure(e, e->part_total, (size_t)spl.nparts * 4)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->part_start, ((size_t)spl.nparts + 1) * 8)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->part_offs32, (size_t)spl.G * spl.nparts * 4)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->recs, (size_t)slots * 8)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->slices, slice_table_bytes(slots, spl))) != TAD_OK) return rc;
    uint32_t *offs32 = static_cast<uint32_t *>(e->part_offs32.p);
    unsigned long long *part_start = static_cast<unsigned long long *>(e->part_start.p);
    launch_part_offsets(s, a.binhist, spl, offs32, static_cast<uint32_t *>(e->part_total.p), part_start, false,
                        static_cast<const MetaPartial *>(e->meta.p), n, slots, e->slices.p, Grid{});
    // (no overflow list: a value that does not fit the record raises DEV_ERR_OVERFLOW_LIST and the LSD sort redoes the job)
    launch_partition(s, j.rows, K, j.rf, L, spl, offs32, part_start, e->recs.p, nullptr, dev_ovf_count(e), 0, j.ctr);
    launch_sparse_sort(s, e->recs.p, part_start, a.binhist, spl, K, L.step, j.op_max,
                       ucomp, static_cast<unsigned long long *>(e->sp_comp_b.p), static_cast<unsigned long long *>(e->sp_val_b.p),
                       reinterpret_cast<uint32_t *>(uval), e->sp_temp.p, ss.d_runs, j.ctr);
  } else if (launch_sparse_group(s, j.rows, K,
                                 j.rf, L.t0, span, j.op_max, ucomp, uval, static_cast<unsigned long long *>(e->sp_comp_b.p),
                                 static_cast<unsigned long long *>(e->sp_val_b.p), e->sp_temp.p, tb, ss.d_runs, j.ctr) != 0)
    return fail(e, TAD_ERR_HIP, "sparse Stage 0: sort / reduce failed");
  if (j.depth == 0) e->sp_by_partition = a.sp_part;
  // (the partition sort counted both numbers itself)
  if (!a.sp_part) sparse_first_tmax(e, j, ss);
  unsigned long long runs_tmax[2] = {0, 0};
  HIP_TRY(e, hipMemcpyAsync(runs_tmax, ss.d_runs, 16, hipMemcpyDeviceToHost, s));
  if (a.sp_part) HIP_TRY(e, hipMemcpyAsync(e->ctr_host, j.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  ss.P = runs_tmax[0];
  ss.tmax = (unsigned int)runs_tmax[1];
  return a.sp_part ? decide(e, j, rs, a, e->ctr_host->err) : TAD_OK;
}

// A sparse streaming batch builds no rank grid and takes no length classes: k_stream_points walks the sorted unique list
// (e->sp_comp_a / e->sp_val_a) itself, from per-key point offsets.  Its cost follows the batch's points plus the state.
int sparse_stream_offsets(JobCtx *e, const Job &j, Attempt &a, const SparseSort &ss) {
  hipStream_t s = e->stream;
  const uint64_t K = j.K;
  int rc;
  sparse_sorted_list(e, j, a, ss);
  if ((rc = ensure_key_buffers(e, K)) != TAD_OK) return rc;
  StreamPoints sp;
  if ((rc = carve_buf(e, e->sp_cls, &sp, stream_points_layout, K)) != TAD_OK) return rc;
  HIP_TRY(e, hipMemsetAsync(sp.len, 0, (size_t)K * 4, s));
  launch_sparse_len(s, ss.ucomp, ss.P, static_cast<const uint32_t *>(e->sp_first.p), sp.len);
  launch_scan(s, sp.len, sp.poff, K, static_cast<unsigned long long *>(e->scan_scratch.p), nullptr);
  a.stream_poff = sp.poff;
  a.stream_P = ss.P;
  a.g = Grid{nullptr, nullptr, K, 0, nullptr};
  HIP_TRY(e, hipEventRecord(e->ev[3], s));
  return TAD_OK;
}

int run_sparse_classes(JobCtx *e, const tad_job *job, const JobParams &jp, bool op_max, uint64_t n_rows_in, uint64_t rows_used, uint64_t K, Lattice L,
                       uint64_t P, uint32_t tmax, tad_mem out_memory, tad_result **out);
int sparse_points_direct(JobCtx *e, uint64_t n_rows_in, uint64_t rows_used, Lattice L, uint64_t P, DevCounters *ctr, tad_mem out_memory,
                         tad_points **points_out);

// The rank grid: K x the longest series, each key's points in time order with their times beside them.  Skewed series lengths (one key with
// a day of seconds next to many short-lived ones): K x Tmax does not fit although the points do — the keys are split into length classes
// that run as jobs of their own (run_sparse_classes), and the job returns from here (a.finished).
int sparse_rank_grid(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a, const SparseSort &ss, tad_result **out, tad_points **points_out) {
  hipStream_t s = e->stream;
  const uint64_t K = j.K, P = ss.P;
  const unsigned int tmax = ss.tmax;
  int rc;
  const uint64_t cells = a.cells = K * (uint64_t)tmax;
  a.need = cells * 17 + (j.jp.algo == TAD_ALGO_ARIMA ? cells * 80 + (1ull << 22) : (j.jp.algo == TAD_ALGO_DROP ? cells * 8 : 0));
  if (P && j.depth == 0 && (a.need > e->ws_limit || j.plan.sparse_classes == 1)) {
    sparse_sorted_list(e, j, a, ss);
    HIP_TRY(e, hipMemcpyAsync(e->ctr_host, j.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    const DevCounters c0 = *e->ctr_host;
    if ((rc = decide(e, j, rs, a, c0.err & (DEV_ERR_KEY_RANGE | DEV_ERR_OFF_LATTICE))) != TAD_OK || a.retry) return rc;
    a.finished = true;
    if (j.points_mode) return sparse_points_direct(e, j.rows.n, c0.rows_used, a.L, P, j.ctr, j.out_memory, points_out);   // Stage 0 alone needs no grid
    return run_sparse_classes(e, j.job, j.jp, j.op_max, j.rows.n, c0.rows_used, K, a.L, P, tmax, j.out_memory, out);
  }
  if (a.need > e->ws_limit)
    return fail(e, TAD_ERR_GRID_TOO_LARGE, "sparse point grid needs %llu bytes (%llu keys x longest series %u points) > workspace limit %llu",
                (unsigned long long)a.need, (unsigned long long)K, tmax, (unsigned long long)e->ws_limit);
  if ((rc = ensure(e, e->grid_val, (cells ? cells : 1) * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->grid_flag, cells ? cells : 1)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->sp_times, (cells ? cells : 1) * 8)) != TAD_OK) return rc;
  a.g = Grid{static_cast<unsigned long long *>(e->grid_val.p), static_cast<uint8_t *>(e->grid_flag.p), tmax ? K : 0, tmax,
             static_cast<const long long *>(e->sp_times.p)};
  if (cells) {
    HIP_TRY(e, hipMemsetAsync(a.g.flag, 0, cells, s));
    if (a.sp_part)
      launch_sparse_place_staged(s, ss.spl, e->sp_temp.p, static_cast<const unsigned long long *>(e->sp_comp_b.p), static_cast<const unsigned long long *>(e->sp_val_b.p),
                                 reinterpret_cast<const uint32_t *>(ss.uval), a.L.t0, a.g, static_cast<long long *>(e->sp_times.p));
    else
      launch_sparse_place(s, ss.ucomp, ss.uval, P, static_cast<const uint32_t *>(e->sp_first.p), a.L.t0, a.g, static_cast<long long *>(e->sp_times.p));
  }
  HIP_TRY(e, hipEventRecord(e->ev[3], s));
  return TAD_OK;
}

int stage0_sparse(JobCtx *e, const Job &j, Stage0Retry &rs, Attempt &a, tad_result **out, tad_points **points_out) {
  SparseSort ss;
  int rc;
  if ((rc = sparse_sort(e, j, rs, a, ss)) != TAD_OK || a.retry) return rc;
  if (j.stream) return sparse_stream_offsets(e, j, a, ss);
  return sparse_rank_grid(e, j, rs, a, ss, out, points_out);
}

// DBSCAN job: pass C in settle mode — key rounds, the detector's per-key pass on the LDS tile, grid columns of unsettled keys only.
// Decided BEFORE pass B: with `max` the tile cells are 32-bit words (value + 1; three key rounds instead of six at C4) and pass B keeps
// values >= 2^32 - 1 out of the records (overflow list + a bitmap of their keys, which alone are left to k_dbscan_scan).
// Sets j.jp.settled and a.narrow_tiles; *ovf_keys: the bitmap for pass B (NULL: no settle mode).
int settle_setup(JobCtx *e, Job &j, const Stage0Retry &rs, Attempt &a, SettleArgs *settle, uint32_t **ovf_keys) {
  hipStream_t s = e->stream;
  const Grid g = a.g;
  int rc;
  *settle = SettleArgs{};
  *ovf_keys = nullptr;
  j.jp.settled = false;
  if (!(j.jp.algo == TAD_ALGO_DBSCAN && !j.jp.all_points && !j.points_mode && !j.stream && dbscan_uses_list(g) &&
        part_plan_settle(a.L.nb, &a.pl, j.op_max && !rs.wide_tiles)))
    return TAD_OK;
  if ((rc = ensure(e, e->aux, dbscan_scratch_bytes(g))) != TAD_OK) return rc;
  if ((rc = ensure(e, e->ovf_keys, ((size_t)(j.K + 31) / 32) * 4 + 64)) != TAD_OK) return rc;
  *ovf_keys = static_cast<uint32_t *>(e->ovf_keys.p);
  HIP_TRY(e, hipMemsetAsync(*ovf_keys, 0, ((size_t)(j.K + 31) / 32) * 4, s));
  unsigned int *cnt = static_cast<unsigned int *>(e->aux.p);
  HIP_TRY(e, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned int), s));    // work-list and redo-list lengths
  settle->redo_list = dbscan_redo_list(g, e->aux.p);
  settle->redo_count = cnt + 1;
  settle->st = DbscanStats{static_cast<uint32_t *>(e->n_pts.p), static_cast<uint32_t *>(e->n_anom.p), static_cast<double *>(e->key_mean.p),
                           static_cast<double *>(e->key_m2.p)};
  settle->list = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(e->aux.p) + 64);
  settle->count = cnt;
  settle->eps = j.jp.eps;
  settle->min_samples = j.jp.min_samples;
  settle->on = 1;
  settle->ovf_keys = *ovf_keys;
  dbscan_compact_series(g, e->aux.p, &settle->cs_val, &settle->cs_flag, &settle->cs_has, &settle->cs_cap);
  dbscan_redo_series(g, e->aux.p, &settle->rs_val, &settle->rs_flag, &settle->rs_has, &settle->rs_cap);
  j.jp.settled = true;
  a.narrow_tiles = a.pl.narrow;
  return TAD_OK;
}

// Stage 0 v2 on the dense grid: pass B partitions the rows into per-tile regions of packed records (sized from a.binhist), pass C
// aggregates every tile in LDS and writes the grid.
int stage0_tiles(JobCtx *e, Job &j, Stage0Retry &rs, Attempt &a) {
  hipStream_t s = e->stream;
  const uint64_t n = j.rows.n, K = j.K;
  PartPlan &pl = a.pl;
  int rc;
  part_plan_wc(a.hist_sampled ? sampled_slots_bound(j.slots_all, pl) : j.slots_all, j.rows.aligned16(), j.has2, j.plan.partition_pass, &pl);
  // nparts is only known now: the bound is recomputed with the final plan (part_plan_bins' G, part_plan_tiles' nparts)
  const uint64_t slots = a.hist_sampled ? sampled_slots_bound(j.slots_all, pl) : j.slots_all + pl.pad_slots;
  {
    Stage0Facts f;
    f.sampled_slots_2_32 = a.hist_sampled && slots >= (1ull << 32);
    if ((rc = decide(e, j, rs, a, f)) != TAD_OK || a.retry) return rc;
  }
  uint32_t *fin = nullptr;
  if (a.hist_sampled) {
    if ((rc = ensure(e, e->part_fin, (size_t)pl.G * pl.nparts * 8)) != TAD_OK) return rc;
    fin = static_cast<uint32_t *>(e->part_fin.p);
  }
  if ((rc = ensure(e, e->part_total, (size_t)pl.nparts * 4)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->part_start, ((size_t)pl.nparts + 1) * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->part_offs32, (size_t)pl.G * pl.nparts * 4)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->recs, (size_t)slots * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->ovf, 16 + (size_t)kOverflowCap * sizeof(OverflowRec))) != TAD_OK) return rc;
  unsigned long long *ovf_count = dev_ovf_count(e);     // in the job tail: zeroed with the counters, one fill per attempt
  OverflowRec *ovf = reinterpret_cast<OverflowRec *>(static_cast<unsigned char *>(e->ovf.p) + 16);
  if ((rc = ensure_key_buffers(e, K)) != TAD_OK) return rc;
  if ((rc = ensure_rcp_table(e, a.L.nb)) != TAD_OK) return rc;
  uint32_t *offs32 = static_cast<uint32_t *>(e->part_offs32.p);
  unsigned long long *part_start = static_cast<unsigned long long *>(e->part_start.p);
  if ((rc = ensure(e, e->slices, slice_table_bytes(slots, pl))) != TAD_OK) return rc;
  launch_part_offsets(s, a.binhist, pl, offs32, static_cast<uint32_t *>(e->part_total.p), part_start,
                      a.hist_sampled, static_cast<const MetaPartial *>(e->meta.p), n, slots, e->slices.p, a.g, j.ctr);
  // (per-key statistics run as their own kernel: fusing them into the tile pass measured slower on MI355X — one
  // wavefront per tile walks a 250-step FP64 dependency chain while the CU's other wavefronts have nothing left to do)
  SettleArgs settle;
  uint32_t *ovf_keys;
  if ((rc = settle_setup(e, j, rs, a, &settle, &ovf_keys)) != TAD_OK) return rc;
  HIP_TRY(e, hipEventRecord(e->ev[2], s));
  launch_partition(s, j.rows, K, j.rf, a.L, pl, offs32, part_start, e->recs.p, ovf, ovf_count, kOverflowCap, j.ctr, fin, ovf_keys);
  HIP_TRY(e, hipEventRecord(e->ev[3], s));
  launch_tile_aggregate(s, e->recs.p, part_start, pl, slots, e->slices.p, a.g, j.op_max, ovf, ovf_count, kOverflowCap,
                        a.hist_sampled ? offs32 : nullptr, fin, settle);
  return TAD_OK;
}

// The dense K x T grid: through the partition + LDS tiles (v2), or zeroed and filled by direct atomics (v1: small batches, the fallback,
// a tile that does not fit LDS).
int stage0_dense(JobCtx *e, Job &j, Stage0Retry &rs, Attempt &a) {
  hipStream_t s = e->stream;
  const uint64_t K = j.K;
  int rc;
  if (a.cells_overflow) return fail(e, TAD_ERR_GRID_TOO_LARGE, "grid of %llu keys x %llu buckets overflows", (unsigned long long)K, (unsigned long long)a.L.nb);
  {
    Stage0Facts f;
    f.grid_too_large = a.need > e->ws_limit;
    if ((rc = decide(e, j, rs, a, f)) != TAD_OK || a.retry) return rc;
  }
  if ((rc = ensure(e, e->grid_val, a.cells * 8)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->grid_flag, a.cells)) != TAD_OK) return rc;
  a.g = Grid{static_cast<unsigned long long *>(e->grid_val.p), static_cast<uint8_t *>(e->grid_flag.p), j.empty ? 0 : K, a.L.nb, nullptr};
  if (a.v2 && !part_plan_tiles(K, a.L.nb, j.has2, &a.pl)) a.v2 = false;  // tile does not fit LDS: direct scatter
  if (a.v2) return stage0_tiles(e, j, rs, a);
  if (a.cells) {
    HIP_TRY(e, hipMemsetAsync(a.g.val, 0, a.cells * 8, s));
    HIP_TRY(e, hipMemsetAsync(a.g.flag, 0, a.cells, s));
  }
  HIP_TRY(e, hipEventRecord(e->ev[2], s));
  if (!j.empty)
    launch_scatter(s, j.rows, j.rf, a.L, a.g, j.op_max, j.ctr);
  HIP_TRY(e, hipEventRecord(e->ev[3], s));
  return TAD_OK;
}

// ---- Stage 1+2: sigma, detector, count, scan ----

// Stage 0 alone: every present point is a row (counts = n_pts)
int count_points(JobCtx *e, const Job &j, const Attempt &a, uint64_t *rows) {
  hipStream_t s = e->stream;
  const Grid g = a.g;
  int rc;
  if ((rc = ensure_key_buffers(e, g.K)) != TAD_OK) return rc;
  if ((rc = ensure_rcp_table(e, g.T)) != TAD_OK) return rc;
  launch_key_sigma(s, g, 0.5, false, static_cast<const double *>(e->rcp_table.p), static_cast<double *>(e->sigma.p),
                   static_cast<uint32_t *>(e->n_pts.p), static_cast<uint32_t *>(e->n_anom.p), j.ctr, static_cast<double *>(e->key_mean.p),
                   static_cast<double *>(e->key_m2.p));
  launch_moments(s, g.K, static_cast<const uint32_t *>(e->n_pts.p), static_cast<const double *>(e->key_mean.p),
                 static_cast<const double *>(e->key_m2.p), dev_moments(e));
  unsigned long long *off = static_cast<unsigned long long *>(e->off.p);
  launch_scan(s, static_cast<const uint32_t *>(e->n_pts.p), off, g.K, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  *rows = *e->total_host;
  return TAD_OK;
}

// what a streaming batch's count pass leaves for its emit
struct StreamBatches {
  HistBatch hist;
  ArimaBatch ab;
  DropBatch db;
};

// One streaming batch: the per-key recurrences continue from the stored state, the next state stays a candidate; a batch on a history /
// series state also merges / appends its points, and DBSCAN, ARIMA and DROP judge them there (tad_capi.cpp).  tad_state_merge places the
// points by time instead: no count pass (it would refuse a late row), no rows.
int count_stream(JobCtx *e, const Job &j, const Attempt &a, StreamBatches *sb, uint64_t *rows) {
  hipStream_t s = e->stream;
  tad_state *stream = j.stream;
  const Grid g = a.g;
  const JobParams &jp = j.jp;
  const uint64_t P_bound = j.slots_all < a.cells ? j.slots_all : a.cells;
  int rc;
  if ((rc = ensure_key_buffers(e, g.K)) != TAD_OK) return rc;
  if (e->merge) {
    e->merge->changed = false;
    if (e->merge->ch && (rc = merge_report_begin(e, stream, e->merge)) != TAD_OK) return rc;
    // (a replace runs for a batch without a live row, a merge does not: a replace's range still erases)
    if ((e->merge->replace ? stream->K : g.K) != 0 &&
        (rc = state_merge_batch(e, stream, g, a.L, a.stream_poff, a.stream_P, P_bound, j.op_max, jp.alpha, e->merge)) != TAD_OK)
      return rc;
  } else if (a.stream_poff)
    launch_stream_points(s, static_cast<const unsigned long long *>(e->sp_comp_a.p), static_cast<const unsigned long long *>(e->sp_val_a.p), a.stream_poff,
                         g.K, a.L.t0, jp.alpha, jp.all_points, false, state_view(stream, stream->cur), state_view(stream, stream->cur ^ 1),
                         static_cast<uint32_t *>(e->n_anom.p), nullptr, OutRows{}, j.ctr);
  else
    launch_stream(s, g, a.L, jp.alpha, jp.all_points, false, state_view(stream, stream->cur), state_view(stream, stream->cur ^ 1),
                  static_cast<uint32_t *>(e->n_anom.p), nullptr, OutRows{}, j.ctr);
  unsigned long long *off = static_cast<unsigned long long *>(e->off.p);
  if (!e->merge && (stream->history || stream->series) && g.K &&
      (rc = stream_history_batch(e, stream, g, a.L, a.stream_poff, a.stream_P, P_bound, jp, &sb->hist)) != TAD_OK)
    return rc;
  if (jp.algo == TAD_ALGO_ARIMA && g.K && (rc = stream_arima_batch(e, series_view(stream, stream->cur ^ 1), sb->hist, jp, j.ctr, &sb->ab)) != TAD_OK) return rc;
  if (jp.algo == TAD_ALGO_DROP && g.K) {   // tad_drop_stream: the touched keys' statistics over the candidate series, the new points' verdicts and rows
    const StateView cv = series_view(stream, stream->cur ^ 1);
    ViewRoute route;   // (hs_kcnt once more, at the size stream_history_batch gave it: nothing grows here)
    if ((rc = carve_buf(e, e->hs_kcnt, &route, view_route_layout, g.K)) != TAD_OK) return rc;
    if ((rc = state_drop_batch(e, cv, sb->hist, jp, true, win_coop_min(g.K, stream->ser.len[stream->cur] + sb->hist.P_cap), route.list, route.lcount,
                               j.ctr, &sb->db)) != TAD_OK)
      return rc;
  }
  if (jp.algo == TAD_ALGO_EWMA && !e->merge)   // (a DBSCAN / ARIMA / DROP batch counted its rows in stream_history_batch / stream_arima_batch)
    launch_scan(s, static_cast<const uint32_t *>(e->n_anom.p), off, g.K, static_cast<unsigned long long *>(e->scan_scratch.p), dev_total(e));
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  HIP_TRY(e, hipGetLastError());
  *rows = *e->total_host;
  for (int b = 0; b < kMomentBlocks; ++b) e->moments_host[b] = Moments{0.0, 0.0, 0.0};
  return TAD_OK;
}

// ---- the results ----

// the Stage-0 part of tad_stats that a points result and a rows result share
void stage0_stats(JobCtx *e, const Job &j, const Attempt &a, const DevCounters &c, int attempts, tad_stats &st) {
  st.rows_in = j.rows.n;
  st.rows_used = c.rows_used;
  st.n_keys = c.n_keys;
  st.n_points = c.n_points;
  st.t0 = a.L.t0; st.step = a.L.step; st.n_buckets = a.L.nb;
  hipEventElapsedTime(&st.ms_meta, e->ev[0], e->ev[1]);
  hipEventElapsedTime(&st.ms_stage0, e->ev[1], e->ev[5]);
  hipEventElapsedTime(&st.ms_scatter, e->ev[2], e->ev[3]);
  hipEventElapsedTime(&st.ms_detect, e->ev[5], e->ev[4]);
  hipEventElapsedTime(&st.ms_total, e->ev[0], e->ev[4]);
  st.stage0_path = a.stage0_path();
  st.stage0_attempts = attempts;
  st.hist_sampled = a.hist_source();
}

// The three columns of a points result (tad_aggregate) in one device block, `stride` entries each.
struct PointsOut {
  PointsPriv *pp = nullptr;
  ResultBlock blk;
  uint64_t stride = 0;
  unsigned char *d = nullptr;
  unsigned long long *key() const { return reinterpret_cast<unsigned long long *>(d); }
  long long *time() const { return reinterpret_cast<long long *>(d + stride * 8); }
  unsigned long long *value() const { return reinterpret_cast<unsigned long long *>(d + stride * 16); }
};

int make_points(JobCtx *e, uint64_t rows, PointsOut *po) {
  po->pp = new (std::nothrow) PointsPriv();
  if (!po->pp) return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  memset(po->pp, 0, sizeof *po->pp);
  po->stride = rows ? rows : 1;
  const int rc = alloc_device_block(e, (size_t)po->stride * 24, &po->blk);
  if (rc != TAD_OK) { delete po->pp; return rc; }
  po->d = static_cast<unsigned char *>(po->blk.base);
  return TAD_OK;
}

void drop_points(JobCtx *e, PointsOut *po) {
  release_block(e, po->blk.base, po->blk.cap);
  delete po->pp;
}

// After the kernels that fill the block are on the stream: the block handed over, or copied to a host block; the call's last
// synchronisation; the tad_points fields.  On failure the block and the result are gone.
int finish_points(JobCtx *e, PointsOut *po, uint64_t rows, tad_mem out_memory) {
  hipStream_t s = e->stream;
  PointsPriv *pp = po->pp;
  const size_t bytes = (size_t)po->stride * 24;
  void *h = nullptr;
  hipError_t hr = hipSuccess;
  if (out_memory == TAD_MEM_HOST) {
    h = malloc(bytes);
    if (!h) { drop_points(e, po); return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory for %zu bytes of points", bytes); }
    hr = hipMemcpyAsync(h, po->d, bytes, hipMemcpyDeviceToHost, s);
  }
  if (hr == hipSuccess) hr = hipStreamSynchronize(s);
  if (hr == hipSuccess) hr = hipGetLastError();
  if (hr != hipSuccess) {
    free(h);
    drop_points(e, po);
    return fail(e, TAD_ERR_HIP, "Stage 0, points: %s", hipGetErrorString(hr));
  }
  unsigned char *base = po->d;
  if (out_memory == TAD_MEM_HOST) {
    release_block(e, po->blk.base, po->blk.cap);
    base = static_cast<unsigned char *>(h);
    pp->block = h; pp->block_cap = bytes;
  } else {
    pp->block = po->blk.base; pp->block_cap = po->blk.cap;
  }
  pp->pub.n_points = rows;
  pp->pub.key_id = reinterpret_cast<uint64_t *>(base);
  pp->pub.flow_end_s = reinterpret_cast<int64_t *>(base + po->stride * 8);
  pp->pub.value = reinterpret_cast<uint64_t *>(base + po->stride * 16);
  pp->pub.memory = out_memory;
  return TAD_OK;
}

// Stage 0 alone (tad_aggregate): the grid's present points as three columns
int job_points(JobCtx *e, const Job &j, const Attempt &a, const DevCounters &c, uint64_t rows, int attempts, tad_points **points_out) {
  hipStream_t s = e->stream;
  PointsOut po;
  int rc;
  if ((rc = make_points(e, rows, &po)) != TAD_OK) return rc;
  if (rows) launch_emit_points(s, a.g, a.L, static_cast<const unsigned long long *>(e->off.p), po.key(), po.time(), po.value());
  const hipError_t er = hipEventRecord(e->ev[4], s);
  if (er != hipSuccess) { drop_points(e, &po); return fail(e, TAD_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(er)); }
  if ((rc = finish_points(e, &po, rows, j.out_memory)) != TAD_OK) return rc;
  tad_stats &st = po.pp->pub.stats;
  stage0_stats(e, j, a, c, attempts, st);
  merge_moments(e->moments_host, a.g.K != 0, &st.pts_mean, &st.pts_m2);
  e->done.store(4);
  *points_out = &po.pp->pub;
  return TAD_OK;
}

// tad_state_merge: no rows; the candidate copies become current together
int job_merge(JobCtx *e, const Job &j, const Attempt &a, const DevCounters &c, int attempts) {
  MergeCall *mc = e->merge;
  tad_state *stream = j.stream;
  HIP_TRY(e, hipEventRecord(e->ev[4], e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  tad_merge_stats &ms = mc->stats;
  ms.rows_in = j.rows.n;
  ms.rows_used = c.rows_used;
  ms.stage0_path = a.stage0_path();
  ms.stage0_attempts = attempts;
  ms.job_context = e->index;
  hipEventElapsedTime(&ms.ms_stage0, e->ev[1], e->ev[5]);
  hipEventElapsedTime(&ms.ms_merge, e->ev[5], e->ev[4]);
  hipEventElapsedTime(&ms.ms_total, e->ev[0], e->ev[4]);
  // a report's host array: staged in context workspace, copied out now that nothing can fail the call any more but this copy (it comes
  // before the candidates become current, so that its failure leaves the state as it was)
  if (mc->ch && mc->ch->key_since && mc->report_staged && stream->K != 0)
    HIP_TRY(e, hipMemcpy(mc->ch->key_since, mc->report.since, (size_t)stream->K * 8, hipMemcpyDeviceToHost));
  if (mc->changed) {
    const int old_cur = stream->cur;
    const uint64_t n_ser = stream->ser.len[old_cur] + mc->added - mc->erased, n_hist = stream->history ? stream->hist.len[old_cur] + mc->added - mc->erased : 0;
    state_commit(stream, n_ser, n_hist);
    // (a replace that erased: the old arenas, now the candidates, are given back when far too big for what is left, as after a trim)
    if (mc->erased) (void)state_size_arenas(e, stream, old_cur, n_ser, n_hist, false, "tad_state_replace");
  }
  if (j.depth == 0) e->done.store(4);
  return TAD_OK;
}

// ---- Stage 3: emit ---- the rows of the job or of the streaming batch, then what the result reports
int job_rows(JobCtx *e, const Job &j, const Attempt &a, const StreamBatches &sb, const DevCounters &c, uint64_t rows, int attempts, tad_result **out) {
  hipStream_t s = e->stream;
  tad_state *stream = j.stream;
  const JobParams &jp = j.jp;
  const Grid g = a.g;
  RowsOut ro;
  int rc;
  if ((rc = make_result(e, rows, jp.all_points, j.out_memory, &ro.rp, &ro.dev_rows, &ro.dev_block)) != TAD_OK) return rc;
  if (rows && stream && jp.algo != TAD_ALGO_EWMA)   // the batch's points as DBSCAN, ARIMA or DROP judged them (stddev: the candidate state's)
    emit_point_rows(s, jp, sb.hist, sb.ab, sb.db, state_view(stream, stream->cur ^ 1), ro.dev_rows);
  else if (rows && stream && a.stream_poff)
    launch_stream_points(s, static_cast<const unsigned long long *>(e->sp_comp_a.p), static_cast<const unsigned long long *>(e->sp_val_a.p), a.stream_poff,
                         g.K, a.L.t0, jp.alpha, jp.all_points, true, state_view(stream, stream->cur), state_view(stream, stream->cur ^ 1),
                         nullptr, static_cast<const unsigned long long *>(e->off.p), ro.dev_rows, j.ctr);
  else if (rows && stream)
    launch_stream(s, g, a.L, jp.alpha, jp.all_points, true, state_view(stream, stream->cur), state_view(stream, stream->cur ^ 1),
                  nullptr, static_cast<const unsigned long long *>(e->off.p), ro.dev_rows, j.ctr);
  else if (rows)
    emit_rows(e, g, a.L, jp, ro.dev_rows, rows);
  if ((rc = finish_rows(e, j.job, &ro, rows, jp.all_points, c, g.K != 0)) != TAD_OK) return rc;
  tad_stats &st = ro.rp->pub.stats;
  stage0_stats(e, j, a, c, attempts, st);
  st.host_syncs = (a.hinted || j.empty) ? 2 : 3;
  if (stream && g.K) {   // the batch succeeded: the candidate state (and history, series) becomes current (an empty batch wrote none)
    unsigned long long added = 0;
    memcpy(&added, e->tail_host + kTailHistLen, 8);
    state_commit(stream, stream->ser.len[stream->cur] + added, stream->hist.len[stream->cur] + added);
  }
  if (j.depth == 0) e->done.store(4);
  *out = &ro.rp->pub;
  return TAD_OK;
}

}  // namespace

namespace tadh {

// the validated job on the context the caller holds; depth > 0: a length class of a skewed sparse table run as a job of its own
int run_job_locked(JobCtx *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out, tad_points **points_out,
                   tad_state *stream, int depth) {
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  if (depth == 0) {
    e->done.store(0);
    e->total.store(4);
    e->arima_relaunches = 0;
  }
  Job j{};
  j.job = job; j.cols = cols; j.stream = stream; j.points_mode = points_out != nullptr; j.depth = depth; j.out_memory = out_memory;
  j.jp = job_params(job);
  j.plan = e->plan;
  j.op_max = job->value_op == TAD_OP_MAX || (job->value_op == TAD_OP_AUTO && job->agg_flow == TAD_AGG_NONE);
  j.has2 = cols->key_id2 != nullptr;
  j.rows.n = cols->n_rows;
  j.K = cols->num_keys;
  j.slots_all = j.rows.n * (j.has2 ? 2 : 1);
  j.rf = RowFilter{job->start_time, job->end_time};
  j.rows.cw = ((job->flags & TAD_FLAG_KEY_U32) ? kColKey32 : 0) | ((job->flags & TAD_FLAG_TIME_U32) ? kColTime32 : 0);
  j.empty = (j.rows.n == 0 || j.K == 0);
  int rc;
  if ((rc = stage_columns(e, j)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->counters, kTailBytes)) != TAD_OK) return rc;
  j.ctr = static_cast<DevCounters *>(e->counters.p);
  HIP_TRY(e, hipEventRecord(e->ev[0], s));
  if (depth == 0) HIP_TRY(e, hipEventRecord(e->ev[6], s));   // (class jobs of a skewed sparse table re-record ev[0..5])

  // what the context's last job learnt about a table of this shape: skip the attempt that is known to fail
  const Stage0Shape shape{j.rows.n, j.K, j.has2, (int)job->algo, (int)j.op_max};
  Stage0Retry rs = Stage0Retry::start(j.plan, cols->n_buckets > 0, depth == 0 ? &e->learnt : nullptr, shape);
  for (int attempt = 1; attempt <= kStage0MaxAttempts; ++attempt) {
    Attempt a;
    HIP_TRY(e, hipMemsetAsync(j.ctr, 0, kTailMoments, s));    // counters, row total, overflow-list count
    j.jp.settled = false;
    if ((rc = derive_lattice(e, j, rs, a)) != TAD_OK) return rc;
    if (a.retry) continue;
    if ((rc = choose_stage0(e, j, rs, a)) != TAD_OK) return rc;
    if (a.retry) continue;
    rc = a.sparse ? stage0_sparse(e, j, rs, a, out, points_out) : stage0_dense(e, j, rs, a);
    if (rc != TAD_OK || a.finished) return rc;
    if (a.retry) continue;
    HIP_TRY(e, hipEventRecord(e->ev[5], s));
    if (depth == 0) e->done.store(2);

    uint64_t rows = 0;
    StreamBatches sb;
    if (j.points_mode) rc = count_points(e, j, a, &rows);
    else if (stream) rc = count_stream(e, j, a, &sb, &rows);
    else rc = detect_and_count(e, a.g, j.jp, j.ctr, &rows);
    if (rc != TAD_OK) return rc;
    const DevCounters c = *e->ctr_host;
    if ((rc = decide(e, j, rs, a, c.err)) != TAD_OK) return rc;
    if (a.retry) continue;
    if (depth == 0) e->done.store(3);

    if (j.points_mode) return job_points(e, j, a, c, rows, attempt, points_out);
    if (e->merge) return job_merge(e, j, a, c, attempt);
    if ((rc = job_rows(e, j, a, sb, c, rows, attempt, out)) != TAD_OK) return rc;
    if (depth == 0 && !stream) rs.learn(j.plan, shape, &e->learnt);
    return TAD_OK;
  }
  return fail(e, TAD_ERR_HIP, "internal error: Stage 0 did not settle on a lattice / strategy after %d attempts", kStage0MaxAttempts);
}

// what every entry point that feeds a batch through run_job_locked checks about the job's Stage-0 fields and the columns (who: the call's
// name in its own messages; the request messages are the reference's wording)
int validate_job_columns(tad_engine *e, const tad_job *job, const tad_columns *cols, const char *who) {
  if (job->agg_flow < TAD_AGG_NONE || job->agg_flow > TAD_AGG_EXTERNAL)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "invalid request: Throughput Anomaly Detector aggregated flow type should be 'pod' or 'external' or 'svc'");
  if (job->start_time != 0 && job->end_time != 0 && job->end_time <= job->start_time)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "invalid request: EndInterval should be after StartInterval");
  if (cols->n_rows > 0 && (!cols->key_id || !cols->flow_end_s || !cols->value))
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: key_id, flow_end_s and value columns are required", who);
  if (cols->n_rows > 0 && cols->num_keys == 0)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: num_keys is 0 but there are rows", who);
  if ((job->flags & TAD_FLAG_KEY_U32) && cols->num_keys >= 0xFFFFFFFFull)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: TAD_FLAG_KEY_U32 needs num_keys < 2^32 - 1 (TAD_KEY_SKIP32 is the skip marker)", who);
  if (cols->n_buckets > 0 && cols->step < 1)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: lattice hint needs step >= 1", who);
  return TAD_OK;
}

}  // namespace tadh

namespace {

// The job (points_out == nullptr), Stage 0 alone (points_out != nullptr), or one streaming batch (stream != nullptr).
int run_job(tad_engine *eng, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out, tad_points **points_out,
            tad_state *stream = nullptr) {
  tad_engine *e = eng;
  const bool points_mode = points_out != nullptr;
  if (stream && e && job && cols) {
    if (job->algo == TAD_ALGO_DBSCAN && !stream->history)
      return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: DBSCAN needs a state with history (tad_state_create_ex with TAD_STATE_HISTORY)");
    if (job->algo == TAD_ALGO_ARIMA && !stream->series)
      return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: ARIMA needs a state with a series (tad_state_create_ex with TAD_STATE_SERIES)");
    if (job->algo != TAD_ALGO_EWMA && job->algo != TAD_ALGO_DBSCAN && job->algo != TAD_ALGO_ARIMA)
      return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: only the EWMA detector has a streaming form, DBSCAN on a state with history and "
                                               "ARIMA on a state with a series (DROP: tad_drop_stream)");
    // k_stream writes the candidate state for keys < cols->num_keys and the double buffer flips as a whole: a batch
    // that declares fewer keys than the state holds would drop the others' state
    if (cols->num_keys != stream->K) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: batch declares %llu keys, the state holds %llu (they must be equal)",
                                                 (unsigned long long)cols->num_keys, (unsigned long long)stream->K);
  }
  if (!e) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_run: engine is NULL");
  if (!job || !cols || (!out && !points_out)) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run: job, cols and out must not be NULL");
  if (out) *out = nullptr;
  if (points_out) *points_out = nullptr;
  if (!points_mode && job->algo != TAD_ALGO_EWMA && job->algo != TAD_ALGO_ARIMA && job->algo != TAD_ALGO_DBSCAN && job->algo != TAD_ALGO_DROP)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "invalid request: Throughput Anomaly Detector algorithm type should be 'EWMA' or 'ARIMA' or 'DBSCAN'");
  {
    const int vrc = validate_job_columns(e, job, cols, "tad_run");
    if (vrc != TAD_OK) return vrc;
  }
  if (job->ewma_alpha < 0.0 || job->ewma_alpha > 1.0 || job->dbscan_eps < 0.0 || job->dbscan_min_samples < 0 || job->arima_maxiter < 0 ||
      job->drop_nsigma < 0.0 || job->drop_min_samples < 0)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run: detector parameter out of range");

  // one job context = one job in flight; a streaming state is advanced by one batch at a time
  std::unique_lock<std::mutex> state_lk;
  if (stream) state_lk = std::unique_lock<std::mutex>(stream->mu);
  if (stream && stream->times_stale)
    return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: the series was imported without its times (tad_state_import_times); state unchanged");
  Lease lease(eng, job->id, !points_mode && job->algo == TAD_ALGO_ARIMA);
  if (!lease.c) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_run: no job context available");
  PauseHold hold(eng);     // (declared after the lease: dropped before the context goes back to the pool)
  lease.c->hold = &hold;
  return run_job_locked(lease.c, job, cols, out_memory, out, points_out, stream, 0);
}

// Stage 0 alone on a sparse table whose rank grid does not fit: the sorted unique points (e->sp_comp_a / e->sp_val_a) are
// the answer — three columns out, counters and moments from the same pass (tad_sparse.hip:k_sparse_points_out).
int sparse_points_direct(JobCtx *e, uint64_t n_rows_in, uint64_t rows_used, Lattice L, uint64_t P, DevCounters *ctr, tad_mem out_memory,
                         tad_points **points_out) {
  hipStream_t s = e->stream;
  int rc;
  if ((rc = ensure(e, e->counters, kTailBytes)) != TAD_OK) return rc;
  PointsOut po;
  if ((rc = make_points(e, P, &po)) != TAD_OK) return rc;
  launch_sparse_points_out(s, static_cast<const unsigned long long *>(e->sp_comp_a.p), static_cast<const unsigned long long *>(e->sp_val_a.p), P, L.t0,
                           po.key(), po.time(), po.value(), dev_moments(e), ctr);
  hipError_t hr = hipMemcpyAsync(e->tail_host, e->counters.p, kTailBytes, hipMemcpyDeviceToHost, s);
  if (hr == hipSuccess) hr = hipEventRecord(e->ev[7], s);
  if (hr != hipSuccess) { drop_points(e, &po); return fail(e, TAD_ERR_HIP, "sparse Stage 0, points: %s", hipGetErrorString(hr)); }
  if ((rc = finish_points(e, &po, P, out_memory)) != TAD_OK) return rc;
  tad_stats &st = po.pp->pub.stats;
  const DevCounters c = *e->ctr_host;
  st.rows_in = n_rows_in; st.rows_used = rows_used; st.n_keys = c.n_keys; st.n_points = c.n_points;
  st.t0 = L.t0; st.step = L.step; st.n_buckets = L.nb;
  merge_moments(e->moments_host, true, &st.pts_mean, &st.pts_m2);
  hipEventElapsedTime(&st.ms_total, e->ev[6], e->ev[7]);
  st.ms_stage0 = st.ms_total;
  st.stage0_path = e->sp_by_partition ? 10 : 7;
  st.stage0_attempts = 1;
  e->done.store(4);
  *points_out = &po.pp->pub;
  return TAD_OK;
}

// A sparse table whose K x Tmax rank grid does not fit (skewed series lengths): the keys are split into classes by series
// length (tad_sparse.hip), every class is handed to run_job_locked as a points table of its own — renumbered dense key ids,
// (key, time) order kept, one row per point, so its Stage 0 only re-sorts what is sorted — and the row sets are merged back in
// ORIGINAL key order.  Detectors are per key, so the rows are the rows of the single-grid run, bit for bit; the job-wide
// moments are Chan-merged in class order (telemetry).  On entry the sorted unique points are in e->sp_comp_a / e->sp_val_a
// (P of them), e->sp_first[k] = first point of key k; the class jobs reuse every engine buffer, so the parent's state moves
// to a block of its own first.
int run_sparse_classes(JobCtx *e, const tad_job *job, const JobParams &jp, bool op_max, uint64_t n_rows_in, uint64_t rows_used, uint64_t K, Lattice L,
                       uint64_t P, uint32_t tmax, tad_mem out_memory, tad_result **out) {
  hipStream_t s = e->stream;
  int rc;
  const uint32_t nclass = sparse_class_count(tmax);
  ClassKeys ck;
  if ((rc = carve_buf(e, e->sp_cls, &ck, class_keys_layout, K)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K ? K : 1) * sizeof(unsigned long long))) != TAD_OK) return rc;
  uint32_t *len = ck.len, *member = ck.member, *pts = ck.pts;
  unsigned long long *key_off = ck.key_off, *pt_off = ck.pt_off;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const unsigned long long *ucomp = static_cast<const unsigned long long *>(e->sp_comp_a.p), *uval = static_cast<const unsigned long long *>(e->sp_val_a.p);
  const uint32_t *first = static_cast<const uint32_t *>(e->sp_first.p);
  HIP_TRY(e, hipMemsetAsync(len, 0, (size_t)K * 4, s));
  launch_sparse_len(s, ucomp, P, first, len);

  // the class tables, class after class
  const uint64_t kmax = K < P ? K : P;   // keys with points
  ResultBlock blk;
  ClassTables ct;
  if ((rc = carve_block(e, &blk, &ct, class_tables_layout, P, kmax)) != TAD_OK) return rc;
  unsigned long long *c_key = ct.key, *c_val = ct.val;
  long long *c_t = ct.t;
  uint32_t *c_map = ct.map;
  struct Cls { uint64_t keys, points, key0, pt0; tad_result *res; };
  std::vector<Cls> cls;
  auto release = [&]() {
    for (Cls &c : cls) if (c.res) { tad_result_free(e->eng, c.res); c.res = nullptr; }
    release_block(e, blk.base, blk.cap);
  };
  uint64_t key0 = 0, pt0 = 0;
  for (uint32_t c = 0; c < nclass; ++c) {
    launch_sparse_class_counts(s, len, K, c, member, pts);
    launch_scan(s, member, key_off, K, scratch);
    launch_scan(s, pts, pt_off, K, scratch);
    unsigned long long kc = 0, pc = 0;
    hipError_t hr = hipMemcpyAsync(&kc, key_off + K, 8, hipMemcpyDeviceToHost, s);
    if (hr == hipSuccess) hr = hipMemcpyAsync(&pc, pt_off + K, 8, hipMemcpyDeviceToHost, s);
    if (hr == hipSuccess) hr = hipStreamSynchronize(s);
    if (hr != hipSuccess) { release(); return fail(e, TAD_ERR_HIP, "length classes: %s", hipGetErrorString(hr)); }
    if (kc == 0) continue;
    launch_sparse_class_columns(s, ucomp, uval, P, first, len, c, key_off, pt_off, L.t0, c_key + pt0, c_t + pt0, c_val + pt0, c_map + key0);
    cls.push_back(Cls{kc, pc, key0, pt0, nullptr});
    key0 += kc;
    pt0 += pc;
  }
  if (pt0 != P || key0 > kmax) { release(); return fail(e, TAD_ERR_HIP, "internal error: length classes cover %llu of %llu points", (unsigned long long)pt0, (unsigned long long)P); }
  {
    const hipError_t hr = hipStreamSynchronize(s);   // the class jobs below overwrite the sort buffers the kernels above read
    if (hr != hipSuccess) { release(); return fail(e, TAD_ERR_HIP, "length classes: %s", hipGetErrorString(hr)); }
  }

  // one job per class (filters are applied, every (key, time) is unique: the operator no longer matters)
  tad_job sub = *job;
  sub.flags &= ~(TAD_FLAG_KEY_U32 | TAD_FLAG_TIME_U32);   // the class columns are the engine's own 8-byte ones
  sub.start_time = 0;
  sub.end_time = 0;
  sub.value_op = op_max ? TAD_OP_MAX : TAD_OP_SUM;
  uint64_t rows = 0;
  for (Cls &c : cls) {
    tad_columns cc;
    memset(&cc, 0, sizeof cc);
    cc.n_rows = c.points;
    cc.num_keys = c.keys;
    cc.key_id = reinterpret_cast<const uint64_t *>(c_key + c.pt0);
    cc.flow_end_s = reinterpret_cast<const int64_t *>(c_t + c.pt0);
    cc.value = reinterpret_cast<const uint64_t *>(c_val + c.pt0);
    cc.memory = TAD_MEM_DEVICE;
    if ((rc = run_job_locked(e, &sub, &cc, TAD_MEM_DEVICE, &c.res, nullptr, nullptr, 1)) != TAD_OK) { release(); return rc; }
    rows += c.res->n_rows;
  }
  e->done.store(3);

  // merge: rows of original key k start at off[k] = rows of all smaller original keys (whatever their class)
  if ((rc = ensure_key_buffers(e, K)) != TAD_OK) { release(); return rc; }
  if ((rc = ensure(e, e->aux, (size_t)(K ? K : 1) * 8)) != TAD_OK) { release(); return rc; }
  uint32_t *cnt = static_cast<uint32_t *>(e->n_anom.p);
  unsigned long long *off = static_cast<unsigned long long *>(e->off.p), *first_row = static_cast<unsigned long long *>(e->aux.p);
  ResultPriv *rp = nullptr;
  OutRows dev_rows;
  ResultBlock dev_block;
  if ((rc = make_result(e, rows, jp.all_points, out_memory, &rp, &dev_rows, &dev_block)) != TAD_OK) { release(); return rc; }
  hipError_t hr = hipMemsetAsync(cnt, 0, (size_t)K * 4, s);
  for (Cls &c : cls)
    launch_class_count_rows(s, reinterpret_cast<const unsigned long long *>(c.res->key_id), c.res->n_rows, c_map + c.key0, cnt, first_row);
  launch_scan(s, cnt, off, K, static_cast<unsigned long long *>(e->scan_scratch.p));
  for (Cls &c : cls) {
    OutRows src{reinterpret_cast<unsigned long long *>(c.res->key_id), reinterpret_cast<long long *>(c.res->flow_end_s), c.res->throughput,
                c.res->algo_calc, c.res->stddev, c.res->anomaly};
    launch_class_gather(s, src, c.res->n_rows, c_map + c.key0, off, first_row, dev_rows);
  }
  if (hr == hipSuccess) hr = hipEventRecord(e->ev[7], s);
  if (hr == hipSuccess) hr = hipStreamSynchronize(s);
  if (hr == hipSuccess) hr = hipGetLastError();
  if (hr != hipSuccess) {
    release_block(e, dev_block.base, dev_block.cap);
    delete rp;
    release();
    return fail(e, TAD_ERR_HIP, "length classes, merge: %s", hipGetErrorString(hr));
  }
  if ((rc = finish_result(e, rp, rows, jp.all_points, dev_block, dev_rows)) != TAD_OK) { delete rp; release(); return rc; }

  tad_stats &st = rp->pub.stats;
  st.rows_in = n_rows_in;
  st.rows_used = rows_used;
  st.t0 = L.t0; st.step = L.step; st.n_buckets = L.nb;
  double mn = 0.0, mean = 0.0, m2 = 0.0;   // Chan merge of the classes' (n_points, mean, M2), class order
  float ms_classes = 0.0f;
  for (const Cls &c : cls) {
    const tad_stats &cs = c.res->stats;
    st.n_keys += cs.n_keys;
    st.n_points += cs.n_points;
    st.n_anomalies += cs.n_anomalies;
    st.keys_no_result += cs.keys_no_result;
    st.kalman_steps += cs.kalman_steps;
    st.arima_fits += cs.arima_fits;
    ms_classes += cs.ms_total;
    const double pn = (double)cs.n_points;
    if (pn == 0.0) continue;
    if (mn == 0.0) { mn = pn; mean = cs.pts_mean; m2 = cs.pts_m2; continue; }
    const double nn = mn + pn, d = cs.pts_mean - mean;
    mean = mean + d * (pn / nn);
    m2 = m2 + cs.pts_m2 + d * d * (mn * pn / nn);
    mn = nn;
  }
  st.pts_mean = mean;
  st.pts_m2 = m2;
  hipEventElapsedTime(&st.ms_total, e->ev[6], e->ev[7]);
  st.ms_detect = ms_classes;                       // the class jobs, each with its own (small) Stage 0
  st.ms_stage0 = st.ms_total - ms_classes;         // sort + reduce + class tables + merge
  st.stage0_path = e->sp_by_partition ? 9 : 6;
  st.stage0_attempts = 1;
  strncpy(rp->pub.id, job->id, sizeof rp->pub.id - 1);
  release();
  e->done.store(4);
  *out = &rp->pub;
  return TAD_OK;
}

}  // namespace

extern "C" {

int tad_run(tad_engine *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out) {
  if (e && !out) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run: job, cols and out must not be NULL");
  return run_job(e, job, cols, out_memory, out, nullptr);
}

int tad_run_stream(tad_engine *e, tad_state *st, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out) {
  if (!e) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: engine is NULL");
  if (!st || !out) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: state and out must not be NULL");
  return run_job(e, job, cols, out_memory, out, nullptr, st);
}

int tad_aggregate(tad_engine *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_points **out) {
  if (e && !out) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_aggregate: job, cols and out must not be NULL");
  return run_job(e, job, cols, out_memory, nullptr, out);
}

}  // extern "C"
