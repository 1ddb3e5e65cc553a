"""The batch job's retry rules (theia_amd/csrc/tad_stage0_retry.h) walked exhaustively on the host: a stand-alone g++ program
includes the header, starts from every state tad_plan and a context's Learnt can produce, and asks Stage0Retry::next about every
combination of attempt facts the driver can present in that state.  No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "tad_stage0_retry.h"
using namespace tadh;
using namespace tad;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static int key(const Stage0Retry &r) { return r.lat_mode | r.v1 << 2 | r.wide_tiles << 3 | r.exact_hist << 4 | r.kh_rejected << 5 | r.sparse_lsd << 6; }
static int flags(const Stage0Retry &r) { return key(r) >> 2; }

// what the driver can present in state r: a fallback that was taken is not in use any more
static bool possible(const Stage0Retry &r, const Stage0Facts &f) {
  if (f.use_kh && (r.kh_rejected || r.lat_mode == 2)) return false;
  if (f.hist_sampled && (r.exact_hist || r.lat_mode == 2 || f.use_kh)) return false;
  if (f.sp_part && (!f.sparse || r.sparse_lsd || r.v1)) return false;
  if (f.narrow_tiles && (r.wide_tiles || !f.v2 || f.sparse)) return false;
  if (f.v2 && r.v1) return false;
  if (f.sampled_slots_2_32 && !f.hist_sampled) return false;
  if (f.sample_no_live_row && r.lat_mode == 0) return false;
  return true;
}

static int longest[128], states = 0;   // state -> retries of the longest chain from it (-1: not walked yet)
static long pairs = 0;

static int walk(const Stage0Retry &r) {
  if (longest[key(r)] >= 0) return longest[key(r)];
  int best = 0;
  const uint32_t bits[6] = {DEV_ERR_KEY_RANGE, DEV_ERR_OFF_LATTICE, DEV_ERR_OVERFLOW_LIST, DEV_ERR_LATE_ROW, DEV_ERR_REGION_FULL, DEV_ERR_SPARSE_ROUND};
  for (int em = 0; em < 64; ++em)
    for (int b = 0; b < 512; ++b) {
      Stage0Facts f;
      for (int i = 0; i < 6; ++i) if (em >> i & 1) f.err |= bits[i];
      f.v2 = b & 1; f.sparse = b >> 1 & 1; f.sp_part = b >> 2 & 1; f.use_kh = b >> 3 & 1; f.hist_sampled = b >> 4 & 1; f.narrow_tiles = b >> 5 & 1;
      f.sample_no_live_row = b >> 6 & 1; f.sampled_slots_2_32 = b >> 7 & 1; f.grid_too_large = b >> 8 & 1;
      if (!possible(r, f)) continue;
      ++pairs;
      Stage0Retry n = r;
      const Stage0Next x = n.next(f);
      if (f.err & DEV_ERR_KEY_RANGE && !f.sample_no_live_row && !f.grid_too_large && !f.sampled_slots_2_32 && !(f.sparse && f.use_kh) &&
          !(f.sp_part && f.hist_sampled))
        CHECK(x.what == Stage0Next::kFail && x.code == TAD_ERR_KEY_RANGE);   // whatever else the error word holds
      if (x.what == Stage0Next::kFail) CHECK(x.code != TAD_OK && x.msg != nullptr);
      if (x.what != Stage0Next::kRetry) { CHECK(key(n) == key(r)); continue; }
      // 1. strictly forward: no flag is cleared, the lattice mode never falls, and something moved
      CHECK((flags(n) & flags(r)) == flags(r) && n.lat_mode >= r.lat_mode && n.lat_mode <= 2 && key(n) != key(r));
      CHECK(n.learnt_exact_hist == r.learnt_exact_hist && n.probing_sampled_hist == r.probing_sampled_hist);
      const int c = 1 + walk(n);
      if (c > best) best = c;
    }
  ++states;
  longest[key(r)] = best;
  return best;
}

static Stage0Facts facts(uint32_t err) { Stage0Facts f; f.err = err; f.v2 = true; return f; }

int main() {
  // every initial state
  int most = 0, starts = 0;
  for (int &x : longest) x = -1;
  const Stage0Shape shape{1u << 23, 1000, false, 0, 1};
  for (int tile_cells = 0; tile_cells < 2; ++tile_cells)
    for (int histogram = 0; histogram < 3; ++histogram)
      for (int sparse_sort = 0; sparse_sort < 3; ++sparse_sort)
        for (int hinted = 0; hinted < 2; ++hinted)
          for (int lt = 0; lt < 7; ++lt) {   // none | another shape | nothing learnt | exact, in use | exact, on probation | wide tiles | both
            tad_plan plan{};
            plan.tile_cells = tile_cells; plan.histogram = histogram; plan.sparse_sort = sparse_sort;
            Stage0Learnt w;
            w.valid = lt != 0;
            w.shape = shape;
            if (lt == 1) w.shape.K++;
            w.exact_hist = lt == 3 || lt == 4 || lt == 6;
            w.exact_uses = lt == 4 ? 8 : 3;
            w.wide_tiles = lt == 5 || lt == 6;
            const Stage0Retry r = Stage0Retry::start(plan, hinted != 0, lt ? &w : nullptr, shape);
            CHECK(r.lat_mode == (hinted ? 0 : 1) && !r.v1 && !r.kh_rejected);
            CHECK(r.wide_tiles == (tile_cells == 1 || lt == 5 || lt == 6));
            CHECK(r.exact_hist == (histogram == 1 || lt == 3 || lt == 6) && r.sparse_lsd == (sparse_sort == 1));
            CHECK(r.learnt_exact_hist == (lt == 3 || lt == 6) && r.probing_sampled_hist == (lt == 4));
            const int c = walk(r);
            if (c > most) most = c;
            ++starts;
          }
  // 2. the attempt bound is the longest chain
  printf("starts %d states %d pairs %ld longest %d attempts, constant %d\n", starts, states, pairs, most + 1, kStage0MaxAttempts);
  CHECK(most + 1 == kStage0MaxAttempts);

  // 3. the chains the GPU tests pin
  const tad_plan zero{};
  {   // sampled -> REGION_FULL -> exact -> done: 2 attempts
    Stage0Retry r = Stage0Retry::start(zero, false, nullptr, shape);
    Stage0Facts f = facts(DEV_ERR_REGION_FULL);
    f.hist_sampled = true;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.exact_hist && !r.kh_rejected);
    CHECK(r.next(facts(0)).what == Stage0Next::kDone);
    Stage0Learnt w;
    r.learn(zero, shape, &w);
    CHECK(w.valid && w.exact_hist && !w.wide_tiles && w.exact_uses == 0 && w.exact_backoff == 8);
    const Stage0Retry again = Stage0Retry::start(zero, false, &w, shape);
    CHECK(again.exact_hist && again.learnt_exact_hist);
  }
  {   // the caller's histogram -> REGION_FULL -> the job counts for itself (and may still sample)
    Stage0Retry r = Stage0Retry::start(zero, false, nullptr, shape);
    Stage0Facts f = facts(DEV_ERR_REGION_FULL);
    f.use_kh = true;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.kh_rejected && !r.exact_hist);
    f = facts(0);
    f.sparse = f.use_kh = true;   // ... as does a sparse table, before any error word is read
    Stage0Retry s = Stage0Retry::start(zero, false, nullptr, shape);
    CHECK(s.next(f).what == Stage0Next::kRetry && s.kh_rejected);
  }
  {   // narrow tiles -> OVERFLOW_LIST -> wide tiles -> OVERFLOW_LIST -> v1 -> OVERFLOW_LIST -> fail
    Stage0Retry r = Stage0Retry::start(zero, false, nullptr, shape);
    Stage0Facts f = facts(DEV_ERR_OVERFLOW_LIST);
    f.narrow_tiles = true;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.wide_tiles && !r.v1);
    CHECK(r.next(facts(DEV_ERR_OVERFLOW_LIST)).what == Stage0Next::kRetry && r.v1);
    Stage0Facts g; g.err = DEV_ERR_OVERFLOW_LIST;
    const Stage0Next x = r.next(g);
    CHECK(x.what == Stage0Next::kFail && x.code == TAD_ERR_HIP);
  }
  {   // hint -> OFF_LATTICE -> derived -> OFF_LATTICE -> exact -> OFF_LATTICE -> fail
    Stage0Retry r = Stage0Retry::start(zero, true, nullptr, shape);
    CHECK(r.lat_mode == 0);
    CHECK(r.next(facts(DEV_ERR_OFF_LATTICE)).what == Stage0Next::kRetry && r.lat_mode == 1);
    CHECK(r.next(facts(DEV_ERR_OFF_LATTICE)).what == Stage0Next::kRetry && r.lat_mode == 2);
    const Stage0Next x = r.next(facts(DEV_ERR_OFF_LATTICE));
    CHECK(x.what == Stage0Next::kFail && x.code == TAD_ERR_HIP);
  }
  {   // KEY_RANGE fails at once, whatever else is set
    Stage0Retry r = Stage0Retry::start(zero, true, nullptr, shape);
    Stage0Facts f = facts(DEV_ERR_KEY_RANGE | DEV_ERR_OFF_LATTICE | DEV_ERR_OVERFLOW_LIST | DEV_ERR_LATE_ROW | DEV_ERR_REGION_FULL | DEV_ERR_SPARSE_ROUND);
    f.narrow_tiles = f.use_kh = true;
    const Stage0Next x = r.next(f);
    CHECK(x.what == Stage0Next::kFail && x.code == TAD_ERR_KEY_RANGE && key(r) == 0);
    // the precedence after it: LATE_ROW, REGION_FULL, OVERFLOW_LIST, OFF_LATTICE
    f.err &= ~DEV_ERR_KEY_RANGE;
    CHECK(r.next(f).code == TAD_ERR_INVALID_ARGUMENT);
    f.err &= ~DEV_ERR_LATE_ROW;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.kh_rejected && !r.wide_tiles && r.lat_mode == 0);
    f.err &= ~DEV_ERR_REGION_FULL;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.wide_tiles && r.lat_mode == 0);
  }
  {   // the sample saw no live row: only the exact pass is believed; the exact pass's word stands
    Stage0Retry r = Stage0Retry::start(zero, false, nullptr, shape);
    Stage0Facts f = facts(0);
    f.sample_no_live_row = true;
    CHECK(r.next(f).what == Stage0Next::kRetry && r.lat_mode == 2);
    CHECK(r.next(f).what == Stage0Next::kDone);
  }
  return 0;
}
"""


def test_every_retry_advances_and_the_attempt_bound_is_the_longest_chain(tmp_path):
    src = tmp_path / "retry_walk.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "retry_walk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "longest" in r.stdout, r.stdout
