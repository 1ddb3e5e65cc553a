// tad_stage0_retry.h — what the batch job (tad_capi_job.cpp: run_job_locked) tries next when an attempt at Stage 0 did not hold: the retry
// state, the ONE function that advances it, and what a context remembers about a table's shape between jobs.  Plain C++ (no HIP, no
// engine types): tests/test_stage0_retry.py walks every reachable state of it in a stand-alone program.
#ifndef THEIA_TAD_STAGE0_RETRY_H
#define THEIA_TAD_STAGE0_RETRY_H

#include <stdint.h>

#include "tad.h"
#include "tad_dev_err.h"

namespace tadh {

// Every transition of Stage0Retry::next sets one of five flags that is never cleared, or raises lat_mode (0 -> 1 -> 2): seven retries
// at the most, so eight attempts cover every path.
constexpr int kStage0MaxAttempts = 8;

// a table's shape as JobCtx::learnt keys it
struct Stage0Shape {
  uint64_t n = 0, K = 0;
  bool has2 = false;
  int algo = 0, op = 0;
  bool operator==(const Stage0Shape &o) const { return n == o.n && K == o.K && has2 == o.has2 && algo == o.algo && op == o.op; }
};

// what the last job of a context learnt about its table, reused when the next job has the same shape (nothing speculative: both only
// skip an attempt that is known to fail)
struct Stage0Learnt {
  bool valid = false;
  Stage0Shape shape;
  bool exact_hist = false;   // the sampled histogram proved too optimistic for this table: go straight to the exact one ...
  uint32_t exact_uses = 0, exact_backoff = 8;   // ... for `exact_backoff` jobs, then the sample is tried again (a sorted table may be followed by
                                                // hashed ones of the same shape); a probe that fails doubles the interval, up to 64
  bool wide_tiles = false;   // 32-bit tile cells overflowed the list for this table: go straight to 8-byte cells
};

// the facts of the attempt that just ran, as far as it got (next() is asked at every point where an attempt can end early)
struct Stage0Facts {
  uint32_t err = 0;               // DevCounters::err as last read back (0 before the attempt's first read)
  bool v2 = false;                // the partition + LDS-tile Stage 0 (pass A ran with its key-bin histogram)
  bool sparse = false;            // the sorted point list instead of the dense grid
  bool sp_part = false;           // ... sorted through the partition pass
  bool use_kh = false;            // pass B's regions are sized from the caller's key-bin histogram
  bool hist_sampled = false;      // ... or from pass A's sample
  bool narrow_tiles = false;      // pass C ran with 32-bit tile cells
  bool sample_no_live_row = false;   // the lattice pass found no live row
  bool sampled_slots_2_32 = false;   // the record slots sized from the sample reach 2^32
  bool grid_too_large = false;       // the dense grid does not fit the workspace
};

struct Stage0Next {
  enum What { kDone, kRetry, kFail } what;
  int code;          // kFail: the TAD_ERR_* code and the message's format (its arguments: Stage0Retry::next)
  const char *msg;
};

struct Stage0Retry {
  // 0: the caller's hint; 1: derived — v2 samples the gcd (pass A) and pass B verifies every row, v1 derives it exactly; 2: exact derivation
  // (k_meta).  A row off the lattice (wrong hint / sample missed a residue) moves to the next mode.
  int lat_mode = 1;
  bool v1 = false;            // the overflow list filled up: Stage 0 v1 (direct atomics)
  bool wide_tiles = false;    // ... under 32-bit tile cells (many values >= 2^32 - 1): 8-byte cells first
  bool exact_hist = false;    // a region sized from pass A's sampled histogram was too small: every row is counted
  bool kh_rejected = false;   // the caller's key-bin histogram did not describe the batch: the job counts for itself
  bool sparse_lsd = false;    // the partition + LDS-sort form of the sparse Stage 0 met a heavy key bin or a value too wide for its records
  bool learnt_exact_hist = false, probing_sampled_hist = false;   // (Stage0Learnt: the exact histogram on the last job's word / the sample on probation)

  // the first attempt's state: the plan's overrides, the caller's lattice hint and (lt != NULL) what the context's last job learnt
  static Stage0Retry start(const tad_plan &plan, bool hinted, const Stage0Learnt *lt, const Stage0Shape &shape) {
    Stage0Retry r;
    r.lat_mode = hinted ? 0 : 1;
    r.wide_tiles = plan.tile_cells == 1;
    r.exact_hist = plan.histogram == 1;
    r.sparse_lsd = plan.sparse_sort == 1;
    if (lt && lt->valid && lt->shape == shape) {
      if (lt->exact_hist) {
        if (lt->exact_uses >= lt->exact_backoff) r.probing_sampled_hist = true;   // time to try the sample again
        else { r.exact_hist = true; r.learnt_exact_hist = true; }
      }
      if (lt->wide_tiles) r.wide_tiles = true;
    }
    return r;
  }

  // after a successful job: what the next job of this shape may skip
  void learn(const tad_plan &plan, const Stage0Shape &shape, Stage0Learnt *w) const {
    const bool exact_now = exact_hist && plan.histogram != 1;
    if (learnt_exact_hist) w->exact_uses++;                                           // same table shape, the exact histogram once more
    else if (probing_sampled_hist) { w->exact_uses = 0; w->exact_backoff = exact_now ? (w->exact_backoff < 64 ? w->exact_backoff * 2 : 64) : 8; }
    else { w->exact_uses = 0; w->exact_backoff = 8; }
    w->valid = true;
    w->shape = shape;
    w->exact_hist = exact_now;
    w->wide_tiles = wide_tiles && plan.tile_cells != 1;
  }

  // What the facts mean: kDone (nothing stands against the attempt so far), kRetry (the state has advanced: run the attempt again) or kFail.
  // The message's arguments: the dense-grid message (TAD_ERR_GRID_TOO_LARGE) takes bytes, keys, buckets, step, workspace limit; every
  // other one takes num_keys (the key-range message prints it).
  Stage0Next next(const Stage0Facts &f) {
    // before any error word is read
    if (f.sample_no_live_row) {
      // pass A only SAMPLES the time column: every live row (not TAD_KEY_SKIP, inside the time window) may sit in an unsampled stretch of a
      // big, mostly filtered table.  "No live row" is only believed from the exact pass.
      if (f.v2 && lat_mode == 1) { lat_mode = 2; return retry(); }
      return done();
    }
    // the sparse sort plans LDS rounds of exactly known sizes from the histogram (k_ss_plan): only pass A's own count is trusted with that
    if (f.sparse && f.use_kh) return once(kh_rejected);
    if (f.sp_part && f.hist_sampled) return once(exact_hist);        // the partition sort needs the exact histogram
    if (f.sampled_slots_2_32) return once(exact_hist);               // 32-bit record offsets
    if (f.grid_too_large) {
      if (lat_mode == 1 && f.v2) { lat_mode = 2; return retry(); }   // a too-fine sampled step cannot happen (it is a multiple of the true one); be safe
      return fail(TAD_ERR_GRID_TOO_LARGE, "dense point grid needs %llu bytes (%llu keys x %llu time buckets, step %lld s) > workspace limit %llu");
    }
    // the error word
    if (f.err & tad::DEV_ERR_KEY_RANGE) return fail(TAD_ERR_KEY_RANGE, "a key id is >= num_keys (%llu) and is not TAD_KEY_SKIP");
    if (f.err & tad::DEV_ERR_LATE_ROW)
      return fail(TAD_ERR_INVALID_ARGUMENT, "tad_run_stream: a row is not newer than the last flowEndSeconds of its key's state; state unchanged");
    if (f.err & tad::DEV_ERR_REGION_FULL) {   // a region sized from the sampled histogram was too small: exact histogram
      if (f.use_kh) return once(kh_rejected);   // ... or the caller's histogram is not this batch's: pass A counts
      if (!exact_hist) return once(exact_hist);
      return fail(TAD_ERR_HIP, "internal error: a partition region overflowed with an exact histogram");
    }
    if (f.sp_part) {   // the partition sort: the lattice first; a heavy key bin / a value wider than the record goes to the LSD sort
      if (f.err & tad::DEV_ERR_OFF_LATTICE) return off_lattice();
      if (f.err & (tad::DEV_ERR_OVERFLOW_LIST | tad::DEV_ERR_SPARSE_ROUND)) return once(sparse_lsd);
    }
    if (f.err & tad::DEV_ERR_OVERFLOW_LIST) {  // more than kOverflowCap values >= 2^49: the packed records do not pay off, use v1
      if (f.narrow_tiles && !wide_tiles) return once(wide_tiles);   // (... or >= 2^32 - 1 under 32-bit tile cells: 8-byte cells first)
      if (!v1) return once(v1);
      return fail(TAD_ERR_HIP, "internal error: overflow list full on the v1 path");
    }
    if (f.err & tad::DEV_ERR_OFF_LATTICE) return off_lattice();
    return done();
  }

 private:
  static Stage0Next done() { return Stage0Next{Stage0Next::kDone, TAD_OK, nullptr}; }
  static Stage0Next retry() { return Stage0Next{Stage0Next::kRetry, TAD_OK, nullptr}; }
  static Stage0Next fail(int code, const char *msg) { return Stage0Next{Stage0Next::kFail, code, msg}; }
  // a one-shot fallback: taken once; asked for again, the attempt it bought did not help
  static Stage0Next once(bool &flag) {
    if (flag) return fail(TAD_ERR_HIP, "internal error: Stage 0 took a fallback and met the same refusal again");
    flag = true;
    return retry();
  }
  Stage0Next off_lattice() {   // wrong hint -> derive; sampled gcd too coarse -> exact
    if (lat_mode < 2) { ++lat_mode; return retry(); }
    return fail(TAD_ERR_HIP, "internal error: a row fell off the derived time lattice");
  }
};

}  // namespace tadh

#endif  // THEIA_TAD_STAGE0_RETRY_H
