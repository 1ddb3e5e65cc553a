// tad_engine.h — PRIVATE header of libtad_mi355x.so's host side: the engine, its pool of job contexts, and what the translation
// units of the C ABI share (tad_engine.cpp: life cycle, pool, memory; tad_capi_job.cpp: the batch job; tad_capi.cpp: what the entry points share and the batches
// on a state; tad_capi_view.cpp: the read-only jobs on a state; tad_capi_state.cpp: the life of a streaming state; tad_capi_ingest.cpp: the ingest entry points; tad_capi_series.cpp: the per-series
// entry points; tad_capi_keydict.cpp: the key dictionary; tad_capi_strdict.cpp: the string dictionary; tad_capi_dict.h: what the ingest encoders share).  HIP only: there is no CPU fallback in this library (the CPU oracle under
// oracle/ is test infrastructure and is never linked or called from here).
//
// Threading (controller.go:199-201 runs four workers, Spark ran one pod per job): an engine owns a small POOL of job
// contexts.  A context is everything one job in flight needs — a HIP stream (two: normal and low priority), its events, its pinned
// read-back blocks and its grow-only workspace buffers — so jobs submitted from different threads run concurrently on the GPU, each
// on its own stream, and never touch each other's memory.  tad_run takes an idle context (creating one up to
// tad_engine_opts.max_jobs_in_flight, else waiting), runs, and gives it back.  Serial callers always get context 0 and see the
// behaviour of the single-mutex engine of ABI <= 11.
#ifndef THEIA_TAD_ENGINE_H
#define THEIA_TAD_ENGINE_H

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "tad_internal.h"
#include "tad_stage0_retry.h"

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

struct FreeBlock {
  void *p;
  size_t cap;
};

struct JobCtx;

struct tad_engine {
  int device = 0;
  uint64_t ws_limit = 0;       // per job in flight
  int max_ctx = 1;
  hipStream_t user_stream = nullptr;   // tad_engine_opts.stream: context 0 runs on it (and the pool has that one context)
  int prio_normal = 0, prio_low = 0, prio_high = 0;   // hipDeviceGetStreamPriorityRange: ARIMA jobs (seconds of FP64) run on the low-priority stream of their
                                       // context so that the short HBM-bound jobs of other contexts are dispatched ahead of their workgroups
  std::mutex mu;               // protects plan, ctxs, the busy flags and last_done / last_total
  std::condition_variable cv;  // a context became idle
  tad_plan plan{};             // plan overrides (tests / A-B measurements); all zero = the engine decides
  std::vector<JobCtx *> ctxs;
  int creating = 0;            // contexts being created outside the lock (counted against max_ctx)
  int32_t last_done = 0, last_total = 0;   // progress of the job that finished last (tad_progress with nothing in flight)
  std::mutex err_mu;           // protects err
  std::string err;
  // Whole-CU jobs vs. the ARIMA fit.  A workgroup of pass B / pass C needs a whole CU; the fit kernel of an ARIMA job in flight on another
  // context keeps every CU populated with long-lived wavefronts, so such a workgroup would wait for the fit's whole grid (212 ms measured)
  // whatever the stream priorities.  pause_count = jobs in flight that are in a whole-CU phase; *pause_dev (DEVICE memory) is 0 / non-zero
  // accordingly, written on the 0 <-> 1 transitions by a 4-byte fill on signal_stream (one stream, under pause_mu: the writes cannot
  // pass each other).  The fit polls it every optimiser cycle and suspends while it is raised (tad_arima.hip); its host loop relaunches it
  // (arima_yield_loop).  The word lives in device memory because 2048 wavefronts polling a page-locked HOST word once per cycle (1.6e7
  // reads/s over the host link) doubled the fit's time (C3 266 -> 492 ms, profiles/r6_a4_*); an agent-scope load from HBM costs nothing
  // measurable.
  std::mutex pause_mu;
  int pause_count = 0;         // under pause_mu (read without it by the fit's host loop: a hint, re-checked by the kernel)
  int *pause_dev = nullptr;
  hipStream_t signal_stream = nullptr;
  std::mutex pool_mu;          // protects free_blocks
  std::vector<FreeBlock> free_blocks;  // recycled device result blocks (a result may be freed from any thread)
};

// The grow-only device scratch of a context: DevBuf members and NOTHING ELSE, so that for_each_buf walks the struct as an array and a new
// buffer is trimmed and freed without being listed anywhere.  The static_assert below only catches a member whose size breaks the
// multiple: a pointer pair or any other 16-byte member would pass it and be walked (and hipFree'd) as a DevBuf.  This comment is the guard.
struct JobBufs {
  DevBuf grid_val, grid_flag, sigma, n_pts, n_anom, off, scan_scratch, calc, counters, meta, aux, key_mean, key_m2;   // counters: the job tail (kTailBytes)
  DevBuf in_key, in_key2, in_te, in_ts, in_val;
  DevBuf rcp_table;           // rcp_table[n] = RN(1/n), n = 0..rcp_n-1
  DevBuf binhist, part_total, part_start, part_offs32, recs, ovf, slices;  // Stage 0 v2 (ovf: 8-byte count + overflow records)
  DevBuf sp_comp_a, sp_comp_b, sp_val_a, sp_val_b, sp_temp, sp_first, sp_times;  // Stage 0 sparse (sort + rank grid)
  DevBuf sp_cls;                                                                  // Stage 0 sparse, length classes: per-key class arrays
  DevBuf hs_key, hs_t, hs_val, hs_sorted, hs_noise, hs_cnt, hs_row, hs_koff, hs_kcnt;   // a history batch: new points, sorted values, verdicts, rows, offsets
  DevBuf wv_key, wv_pts;   // tad_run_state_window's view: per key (bounds, offsets, moments) | per window point (values, times, sorted values)
  DevBuf sn_key, sn_pts;   // tad_run_state_since / tad_drop_state_since: per key (the reported suffix, a staged key_since) | per reported point (key, value, time)
  DevBuf bk_key;           // tad_run_state_buckets: per key (buckets, folded points, bucket offsets) | per chunk (heads, their scan); the buckets themselves: wv_pts; tad_state_rollup: its RollupKeys
  DevBuf mg_pts, mg_keys, mg_hist;   // tad_state_merge: per batch point | per key | the history between its subtract and its merge
  DevBuf rp_keys, rp_loss;           // tad_state_replace, beside a merge's: per key (the erased runs) | the values the history loses, packed and sorted
  DevBuf mg_report;                  // tad_state_merge_changes / tad_state_replace_changes: the report's counters | a host array's staging
  DevBuf as_key, as_pt, as_ser, as_fit, as_pos, as_ws;   // a stream ARIMA batch: per key | per new point | packed series | per fit | per position | fit workspace
  DevBuf ds_key, ds_pt;   // tad_drop_state / tad_drop_stream: per key (mean, std, m2, n, ok) | per judged point (verdict, rows, row offset)
  DevBuf dsel;            // tad_drop_select: row bitmask | tile counts | tile offsets | scan scratch | total | a host table's staged columns
  DevBuf part_fin;                                                                // Stage 0 v2, sampled histogram: final cursors of the (workgroup, partition) regions
  DevBuf ovf_keys;                                                                // Stage 0 v2, settle mode: bitmap of the keys with a value on the overflow list
};
static_assert(std::is_standard_layout<JobBufs>::value && sizeof(JobBufs) % sizeof(DevBuf) == 0, "JobBufs holds DevBuf members only");

// One job in flight.  Everything below is touched by the thread that holds the context only (busy == true), except done / total / id.
struct PauseHold;
struct JobCtx : JobBufs {
  tad_engine *eng = nullptr;
  PauseHold *hold = nullptr;   // the running job's claim on whole CUs (run_job); NULL for the small entry points
  int index = 0;               // position in eng->ctxs (tad_stats.job_context)
  bool busy = false;           // under eng->mu
  int device = 0;
  hipStream_t stream = nullptr;        // the stream of the running job: stream_normal or stream_low
  hipStream_t stream_normal = nullptr, stream_low = nullptr;
  bool own_streams = false;
  uint64_t ws_limit = 0;
  tad_plan plan{};             // the engine's plan when the job was admitted
  std::atomic<int32_t> done{0}, total{0};
  char id[64] = {};            // tad_job.id of the running job (tad_job_progress); under eng->mu
  uint64_t rcp_n = 0;             // entries of rcp_table
  struct MergeCall *merge = nullptr;   // set while the context runs a tad_state_merge batch (run_job_locked's merge mode)
  int arima_relaunches = 0;       // times the running job's ARIMA fit was relaunched after it had yielded to whole-CU jobs (tad_stats.arima_relaunches)
  bool sp_by_partition = false;   // the running job's sparse Stage 0 went through the partition pass + LDS sort (stage0_path 8 / 9 / 10 instead of 4 / 6 / 7)
  hipEvent_t ev[8] = {};
  tad::MetaPartial *meta_host = nullptr;    // pinned
  // The job's tail — what the host reads when a job's kernels are done — is ONE block on the device (e->counters: DevCounters |
  // row total | overflow-list count | pad to 128 B | kMomentBlocks moment partials) and ONE pinned block here: one copy per job.
  unsigned char *tail_host = nullptr;        // pinned, kTailBytes
  tad::DevCounters *ctr_host = nullptr;           // = tail_host
  unsigned long long *total_host = nullptr;  // = tail_host + 64
  tad::Moments *moments_host = nullptr;           // = tail_host + 128
  tadh::Stage0Learnt learnt;   // what the last job of this context learnt about its table (tad_stage0_retry.h)
};

// one tad_state_merge or tad_state_replace call: what run_job_locked's merge mode needs beyond the job, and what it reports
struct MergeCall {
  int64_t keep_from = 0;
  tad_merge_stats stats{};   // (a replace: points_combined = the replaced points)
  bool changed = false;    // the candidate copies hold the merged state (false: nothing to merge, the state stays as it is)
  uint64_t added = 0;      // series points gained (inserted + appended)
  // tad_state_replace: the mode, its range (from_t / to_t 0 = no bound on that side) and what it reports beyond a merge
  bool replace = false, ranged = false;
  int64_t from_t = 0, to_t = 0;
  uint64_t erased = 0;     // series points lost: old points inside the range that the batch does not name
  uint64_t emptied = 0;    // keys that held points and hold none afterwards
  // tad_state_merge_changes / tad_state_replace_changes: the caller's report (NULL: none is made) and, per attempt, where the kernels
  // write it (merge_report_begin) and what they counted
  tad_changes *ch = nullptr;
  tad::MergeReport report{};
  bool report_staged = false;   // report.since is context workspace: copied to ch->key_since when the call has succeeded
  tad::ChangeCounters counted{};
};

// A double-buffered value arena of a streaming state: two device arrays of T and their capacities in values, indexed like
// tad_state::block[] by cur / cur ^ 1.  Arenas grow geometrically and are kept; a plain state allocates none.
template <typename T> struct Arena {
  T *p[2] = {nullptr, nullptr};
  uint64_t cap[2] = {0, 0};
  void swap() { std::swap(p[0], p[1]); std::swap(cap[0], cap[1]); }
};

// every key's values as one segment each: off[i] (K + 1 entries) into val.p[i] (val.cap[i] entries, len[i] used)
struct Segments {
  unsigned long long *off[2] = {nullptr, nullptr};
  uint64_t len[2] = {0, 0};
  Arena<unsigned long long> val;
};

// per-key running state of the streaming EWMA detector: two copies (the count pass writes the candidate next state,
// it becomes current only when the batch succeeds)
struct tad_state {
  uint64_t K = 0;
  void *block[2] = {nullptr, nullptr};
  int cur = 0;
  // TAD_STATE_HISTORY: every key's aggregated point values, ascending per key — hist.off[i] (K + 1 entries) and hist.val.p[i] (hist.val.cap[i]
  // entries, hist.len[i] used).  Double-buffered with the same index as block[]: a batch merges into the candidate (cur ^ 1), which
  // becomes current with the moments.  Arenas grow geometrically and are kept; a plain state allocates none of this.
  bool history = false;
  Segments hist;
  // TAD_STATE_SERIES: every key's aggregated point values in time order — ser.off[i] (K + 1 entries) and ser.val.p[i]; the same double
  // buffering and growth as the history (a batch writes old segment ++ new points into the candidate)
  bool series = false;
  Segments ser;
  // TAD_STATE_TIMES (with a series): every series point's flowEndSeconds, parallel to ser.val (same offsets ser.off[i], same lengths, same
  // double buffering; its own capacity).  times_stale: tad_state_import_series replaced the series and tad_state_import_times has not yet
  // brought the times that go with it — batches, trims and exports of the times are refused until it has.
  bool times = false, times_stale = false;
  Arena<long long> ser_times;
  mutable std::mutex mu;     // batches of one state are serial (tad_run_stream from two threads on one state)
};

// A job's claim on whole CUs: raised when its Stage 0 takes the partition path, dropped while its own ARIMA fit runs, dropped for good when
// the job returns.
struct PauseHold {
  tad_engine *eng;
  bool held = false;
  explicit PauseHold(tad_engine *e) : eng(e) {}
  void acquire() {
    if (held || !eng->pause_dev) return;
    std::lock_guard<std::mutex> lk(eng->pause_mu);
    if (eng->pause_count++ == 0) (void)hipMemsetAsync(eng->pause_dev, 1, 4, eng->signal_stream);
    held = true;
  }
  void release() {
    if (!held) return;
    std::lock_guard<std::mutex> lk(eng->pause_mu);
    if (--eng->pause_count == 0) (void)hipMemsetAsync(eng->pause_dev, 0, 4, eng->signal_stream);
    held = false;
  }
  ~PauseHold() { release(); }
  PauseHold(const PauseHold &) = delete;
  PauseHold &operator=(const PauseHold &) = delete;
};

namespace tadh {
using namespace tad;

extern thread_local std::string g_static_err;   // tad_last_error(NULL): the message of a failed tad_engine_create

// the job tail: what the host reads when a job's kernels are done, ONE block on the device and one pinned block on the host
constexpr size_t kTailCtr = 0, kTailTotal = 64, kTailOvfCount = 72, kTailHistLen = 80, kTailMoments = 128;   // kTailHistLen: a history batch's new points
constexpr size_t kTailBytes = kTailMoments + sizeof(Moments) * kMomentBlocks;
inline unsigned long long *dev_total(JobCtx *e) { return reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->counters.p) + kTailTotal); }
inline unsigned long long *dev_ovf_count(JobCtx *e) { return reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(e->counters.p) + kTailOvfCount); }
inline Moments *dev_moments(JobCtx *e) { return reinterpret_cast<Moments *>(static_cast<unsigned char *>(e->counters.p) + kTailMoments); }

constexpr int kMetaBlocks = 2048;
constexpr int kSampleBlockShift = 7;   // (C4 with 1024-key blocks and a sampled histogram: pass A 0.21 -> 0.10 ms but pass C 0.68 -> 0.86 ms, profiles/r3_v2_c4_keyblock_ab.log)
constexpr int kDefaultJobsInFlight = 4;   // controller.go:199-201 / pkg/controller/util.go:43: four workers
constexpr int kMaxJobsInFlight = 16;
constexpr uint32_t kOverflowCap = 1u << 20;  // Stage 0 v2: rows with a value >= 2^49 per run before falling back to v1

bool plan_ok(const tad_plan &p);
int fail(tad_engine *e, int code, const char *fmt, ...);
int fail(JobCtx *c, int code, const char *fmt, ...);
int fail(std::nullptr_t, int code, const char *fmt, ...);

#define HIP_TRY(e, call)                                                                         \
  do {                                                                                           \
    hipError_t err__ = (call);                                                                   \
    if (err__ != hipSuccess)                                                                     \
      return fail((e), err__ == hipErrorOutOfMemory ? TAD_ERR_OUT_OF_MEMORY : TAD_ERR_HIP,       \
                  "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
  } while (0)


// every grow-only buffer of a context, for trimming and teardown
template <typename F> void for_each_buf(JobCtx *c, F f) {
  DevBuf *bufs = reinterpret_cast<DevBuf *>(static_cast<JobBufs *>(c));
  for (size_t i = 0; i < sizeof(JobBufs) / sizeof(DevBuf); ++i) f(bufs[i]);
}

void drop_buffers(JobCtx *c);
void trim_idle(tad_engine *eng, JobCtx *self);
int ensure(JobCtx *e, DevBuf &b, size_t bytes);          // grow-only device scratch
// A workspace block with more than one array (tad_carve.h): its layout function measures it with a walker that has no base, the buffer
// grows, the same function places the arrays.  carve_bufs: a layout over two buffers (per-key counts, per-key offsets).
template <typename L, typename... A, typename... D> size_t carved_bytes(L (*layout)(Carve &, A...), D... dims) {
  Carve m(nullptr);
  layout(m, dims...);
  return m.bytes();
}
template <typename L, typename... A, typename... D> L carve_at(void *base, L (*layout)(Carve &, A...), D... dims) {
  Carve c(base);
  return layout(c, dims...);
}
template <typename L, typename... A, typename... D> int carve_buf(JobCtx *e, DevBuf &b, L *out, L (*layout)(Carve &, A...), D... dims) {
  const int rc = ensure(e, b, carved_bytes(layout, dims...));
  if (rc == TAD_OK) *out = carve_at(b.p, layout, dims...);
  return rc;
}
template <typename L, typename... A, typename... D>
int carve_bufs(JobCtx *e, DevBuf &b0, DevBuf &b1, L *out, L (*layout)(Carve &, Carve &, A...), D... dims) {
  Carve m0(nullptr), m1(nullptr);
  layout(m0, m1, dims...);
  int rc;
  if ((rc = ensure(e, b0, m0.bytes())) != TAD_OK || (rc = ensure(e, b1, m1.bytes())) != TAD_OK) return rc;
  Carve c0(b0.p), c1(b1.p);
  *out = layout(c0, c1, dims...);
  return TAD_OK;
}
// hipMalloc that gives the idle contexts' buffers and the recycled result blocks back to the device (trim_idle) before it fails; *p = NULL then
hipError_t dev_alloc(JobCtx *e, void **p, size_t bytes);
// the refusal of a call whose scratch would pass the workspace limit: "<who> needs <need> bytes of scratch > workspace limit <limit><suffix>"
int over_limit(JobCtx *e, const char *who, size_t need, const char *suffix = "");
void preload_code_objects();
JobCtx *ctx_create(tad_engine *eng, bool first);
void ctx_destroy(JobCtx *c);

// An idle context (the lowest-numbered one: a serial caller always gets context 0 and its warm buffers), a new one while the pool may
// grow, else wait.  low_priority: the job's kernels go to the context's low-priority stream (ARIMA).
struct Lease {
  tad_engine *eng;
  JobCtx *c = nullptr;
  Lease(tad_engine *eng_, const char *id = nullptr, bool low_priority = false) : eng(eng_) {
    std::unique_lock<std::mutex> lk(eng->mu);
    for (;;) {
      for (JobCtx *x : eng->ctxs)
        if (!x->busy) { c = x; break; }
      if (c) break;
      if ((int)eng->ctxs.size() + eng->creating < eng->max_ctx) {
        ++eng->creating;
        lk.unlock();      // (stream / pinned-memory creation outside the lock)
        hipSetDevice(eng->device);
        JobCtx *n = ctx_create(eng, false);
        lk.lock();
        --eng->creating;
        if (n) { n->index = (int)eng->ctxs.size(); eng->ctxs.push_back(n); c = n; break; }
        if (eng->ctxs.empty()) return;   // cannot happen (context 0 is made by tad_engine_create); c stays NULL
      }
      eng->cv.wait(lk);
    }
    c->busy = true;
    c->plan = eng->plan;
    c->done.store(0);
    c->total.store(0);
    memset(c->id, 0, sizeof c->id);
    if (id) strncpy(c->id, id, sizeof c->id - 1);
    c->stream = low_priority ? c->stream_low : c->stream_normal;
    c->hold = nullptr;
  }
  ~Lease() {
    if (!c) return;
    {
      std::lock_guard<std::mutex> lk(eng->mu);
      if (c->total.load() != 0) { eng->last_done = c->done.load(); eng->last_total = c->total.load(); }
      c->busy = false;
      c->id[0] = 0;
      c->hold = nullptr;
    }
    eng->cv.notify_one();
  }
  Lease(const Lease &) = delete;
  Lease &operator=(const Lease &) = delete;
};


// How every call on a state that needs a job context starts: the state's mutex FIRST (the constructor), then — after whatever the call
// refuses or answers from the host alone — a context (enter).  One order for all: a thread that waits for a context never holds one, so
// a call on a busy state cannot keep the pool's last context from the batch that holds the state.  The context goes back before the
// state is unlocked.  who: the call's name in its messages.
struct StateCall {
  tad_engine *eng;
  std::unique_lock<std::mutex> state_lk;
  std::optional<Lease> lease;
  JobCtx *e = nullptr;
  StateCall(tad_engine *eng_, const tad_state *st) : eng(eng_), state_lk(st->mu) {}
  int enter(const char *who, const char *id = nullptr, bool low_priority = false) {
    lease.emplace(eng, id, low_priority);
    e = lease->c;
    if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "%s: no job context available", who);
    HIP_TRY(e, hipSetDevice(e->device));
    return TAD_OK;
  }
};

// recycled device result blocks (engine-wide: a result is freed by whoever holds it)
void release_block(tad_engine *eng, void *p, size_t cap);
inline void release_block(JobCtx *e, void *p, size_t cap) { release_block(e->eng, p, cap); }

uint64_t host_gcd(uint64_t a, uint64_t b);

struct ResultBlock {
  void *base = nullptr;
  size_t cap = 0;
};

int alloc_device_block(JobCtx *e, size_t bytes, ResultBlock *rb);
// a recycled or new device block of the layout's size, and its arrays
template <typename L, typename... A, typename... D> int carve_block(JobCtx *e, ResultBlock *rb, L *out, L (*layout)(Carve &, A...), D... dims) {
  const int rc = alloc_device_block(e, carved_bytes(layout, dims...), rb);
  if (rc == TAD_OK) *out = carve_at(rb->base, layout, dims...);
  return rc;
}

struct ResultPriv {  // lives right behind the public struct
  tad_result pub;
  void *block;
  size_t block_cap;
};

struct PointsPriv {  // tad_points + its storage
  tad_points pub;
  void *block;
  size_t block_cap;
};

struct DropRowsPriv {  // tad_drop_rows + its storage
  tad_drop_rows pub;
  void *block;
  size_t block_cap;
};

struct JobParams {
  tad_algo algo;
  double alpha, eps;
  int min_samples, maxiter;
  double drop_nsigma;
  int drop_min_samples;
  bool all_points;
  bool lazy_sigma = false;   // set by detect_and_count: the stddev column is computed by the emit kernel (DBSCAN jobs)
  bool settled = false;      // set by Stage 0: pass C ran in settle mode (SettleArgs) — the DBSCAN scan only walks the keys it marked
};

// (tad_capi.cpp) shared with the per-series entry points
int ensure_rcp_table(JobCtx *e, uint64_t T);
int ensure_key_buffers(JobCtx *e, uint64_t K);
void emit_rows(JobCtx *e, Grid g, Lattice L, const JobParams &jp, OutRows out, uint64_t rows = 0);

// (tad_capi.cpp) shared with the batch job (tad_capi_job.cpp)
JobParams job_params(const tad_job *job);   // the job's detector parameters, 0 = the reference's default
// the fixed-order Chan merge of the job tail's kMomentBlocks moment partials (any == false: no point, both 0)
void merge_moments(const Moments *blocks, bool any, double *pts_mean, double *pts_m2);
struct RowsOut {   // a rows result in the making: the device block the emit kernels write
  ResultPriv *rp = nullptr;
  OutRows dev_rows{};
  ResultBlock dev_block;
};
int make_result(JobCtx *e, uint64_t rows, bool with_anomaly, tad_mem out_memory, ResultPriv **out, OutRows *dev_rows, ResultBlock *dev_block);
int finish_result(JobCtx *e, ResultPriv *rp, uint64_t rows, bool with_anomaly, ResultBlock dev_block, OutRows dev_rows);
// After the emit kernels are on the stream: ev[4], the block handed over or copied to the host (finish_result), the call's last
// synchronisation — on failure the block and the result are gone — then what every rows result reports: the counters of c, the moments
// (any_points), n_anomalies (TAD_FLAG_EMIT_ALL_POINTS: the verdicts counted), the context, the id.
int finish_rows(JobCtx *e, const tad_job *job, RowsOut *ro, uint64_t rows, bool with_anomaly, const DevCounters &c, bool any_points);

// What a stream ARIMA batch leaves for its emit (stream_arima_batch)
struct ArimaBatch {
  uint64_t P = 0;
  const unsigned long long *tidx = nullptr;    // slot of key k
  const double *sigma = nullptr;               // per slot
  const double *pcalc = nullptr;               // per new point
  const uint8_t *pflag = nullptr;
  const uint32_t *rows = nullptr;
  const unsigned long long *row_off = nullptr;
};
// What the drop detector on a state leaves for its emit (state_drop_batch)
struct DropBatch {
  DropStateKeys keys{};
  const uint8_t *flag = nullptr;
  const uint32_t *cnt = nullptr;
  const unsigned long long *row = nullptr;
};
// (tad_capi.cpp) shared by the stream batch and the read-only jobs on a state (tad_capi_view.cpp): DBSCAN's verdicts and rows of the points hb
// names against a history, filling hb->noise / cnt / row; the emit of the rows of points that DBSCAN, ARIMA or DROP judged
int hist_verdicts(JobCtx *e, const unsigned long long *hoff, const unsigned long long *hval, const JobParams &jp, HistBatch *hb);
void emit_point_rows(hipStream_t s, const JobParams &jp, const HistBatch &hb, const ArimaBatch &ab, const DropBatch &db, const StreamState &mom,
                     OutRows out);
int stream_history_batch(JobCtx *e, tad_state *st, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, uint64_t P_bound,
                         const JobParams &jp, HistBatch *hb);
// a call with a report, before its batch is placed (every attempt, a batch without a live row too): the report's block, every entry
// TAD_NO_CHANGE, the counters at their start
int merge_report_begin(JobCtx *e, const tad_state *st, MergeCall *mc);
// tad_state_merge and tad_state_replace (mc->replace) in the count pass's place; K = the state's keys: a replace runs for a batch
// without a live row too (g.K == 0), which still erases the range
int state_merge_batch(JobCtx *e, tad_state *st, Grid g, Lattice L, const unsigned long long *sparse_poff, uint64_t P, uint64_t P_bound, bool op_max,
                      double alpha, MergeCall *mc);
int stream_arima_batch(JobCtx *e, const StateView &v, const HistBatch &hb, const JobParams &jp, DevCounters *ctr, ArimaBatch *ab);
int state_drop_batch(JobCtx *e, const StateView &v, const HistBatch &hb, const JobParams &jp, bool touched_only, unsigned long long coop_min,
                     uint32_t *list, unsigned int *lcount, DevCounters *ctr, DropBatch *db);

// (tad_capi_job.cpp) the batch job on the context the caller holds, and what every entry point that feeds it a batch checks first
int run_job_locked(JobCtx *e, const tad_job *job, const tad_columns *cols, tad_mem out_memory, tad_result **out, tad_points **points_out,
                   tad_state *stream, int depth);
int validate_job_columns(tad_engine *e, const tad_job *job, const tad_columns *cols, const char *who);

// The ARIMA fit yields to whole-CU jobs of other contexts (PauseHold): its wavefronts suspend their fits while the engine's pause word is raised
// and the kernel is relaunched here — after the word has cleared, or after 2 ms at the latest, so that a steady stream of short jobs
// time-slices with the fit instead of starving it.  relaunch(grace, &yielded_dev) launches the fit again over what it left (0 on success).
template <typename Relaunch>
int arima_yield_loop(JobCtx *e, const unsigned int *yielded_dev, Relaunch relaunch) {
  hipStream_t s = e->stream;
  while (yielded_dev != nullptr && e->eng->pause_dev != nullptr) {
    unsigned int y = 0;
    HIP_TRY(e, hipMemcpyAsync(&y, yielded_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    if (y == 0) break;
    const auto t0 = std::chrono::steady_clock::now();
    while (__atomic_load_n(&e->eng->pause_count, __ATOMIC_ACQUIRE) != 0 && std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(2))
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    // still raised after 2 ms (short jobs arrive back to back): this launch runs 24 optimiser cycles (~1 ms) before it looks at the word
    const uint32_t grace = __atomic_load_n(&e->eng->pause_count, __ATOMIC_ACQUIRE) != 0 ? 24u : 0u;
    if (relaunch(grace, &yielded_dev) != 0) return fail(e, TAD_ERR_HIP, "ARIMA launch failed");
    e->arima_relaunches++;
  }
  return TAD_OK;
}

// (tad_capi_state.cpp) shared with the batches on a state (tad_capi.cpp) and the read-only jobs on it (tad_capi_view.cpp)
inline size_t state_bytes(uint64_t K) { return carved_bytes(stream_state_layout, K); }                          // one block of K keys' running state
inline StreamState stream_view(void *block, uint64_t K) { return carve_at(block, stream_state_layout, K); }     // the arrays inside such a block
StreamState state_view(const tad_state *st, int which);
StateView series_view(const tad_state *st, int which);       // copy `which` as the detectors of tad_run_state read it
int state_grow_candidates(JobCtx *e, tad_state *st, uint64_t P_cap);   // room for a batch of at most P_cap new points
void state_commit(tad_state *st, uint64_t n_ser, uint64_t n_hist); // the candidate copies become current
// copy `i` of every arena sized for n_ser / n_hist values by tad_state_trim's rule: below a quarter of its capacity it is given back and,
// with `allocate`, allocated anew at twice the length
int state_size_arenas(JobCtx *e, tad_state *st, int i, uint64_t n_ser, uint64_t n_hist, bool allocate, const char *who);
uint64_t state_device_bytes(const tad_state *st);            // tad_state_bytes with the state's lock held

}  // namespace tadh

#endif  // THEIA_TAD_ENGINE_H
