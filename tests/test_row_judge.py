"""The row judges of Stage 0 (theia_amd/csrc/tad_rows.h) checked on the host: a stand-alone g++ program includes the header alone and
checks lattice_bucket against plain 128-bit integer arithmetic for lattices that make_lattice builds in all three modes, lattice_bucket_fast
against lattice_bucket wherever the mode is 0 or 1, time_kept at the edges of the time window, the lattice accumulator's merge on random
splits of one list of times, and the key-slot judge at the ends of the key range.  The same program runs clean under the address and
undefined-behaviour sanitizers.  No GPU, no library."""
import os
import subprocess

import pytest
from job_helpers import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tad_rows.h"
using namespace tad;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

typedef __int128 i128;
static const i128 kMin = INT64_MIN, kMax = INT64_MAX;
static long n_bucket[3] = {0, 0, 0}, n_fast = 0, n_merge = 0;

// what the lattice means, in integers that cannot wrap: t is on it when t = t0 + step * b with 0 <= b < nb
static bool ref_bucket(const Lattice &L, int64_t te, uint64_t *b) {
  const i128 d = (i128)te - (i128)L.t0;
  if (d < 0 || d % (i128)L.step != 0) return false;
  const i128 q = d / (i128)L.step;
  if (q >= (i128)L.nb) return false;
  *b = (uint64_t)q;
  return true;
}

static void check_time(const Lattice &L, i128 t) {
  if (t < kMin || t > kMax) return;   // not a time a column can hold
  const int64_t te = (int64_t)t;
  uint64_t want = 0, got = ~0ull, fast = ~0ull;
  const bool on = ref_bucket(L, te, &want);
  CHECK(lattice_bucket(L, te, got) == on);
  if (on) CHECK(got == want);
  else CHECK(got == ~0ull);           // an off-lattice time leaves the bucket alone
  ++n_bucket[L.mode];
  if (L.mode == 2) return;
  CHECK(lattice_bucket_fast(L, te, fast) == on);
  if (on) CHECK(fast == want);
  ++n_fast;
}

// the lattice (t0, step, nb) — a valid one: its last bucket is a time — at every edge
static void check_lattice(int64_t t0, int64_t step, uint64_t nb, int want_mode) {
  if (nb > 0 && (i128)t0 + (i128)(nb - 1) * step > kMax) { CHECK(false); }
  const Lattice L = make_lattice(t0, step, nb);
  CHECK(L.t0 == t0 && L.step == step && L.nb == nb);
  CHECK(L.mode == want_mode);
  const i128 last = (i128)t0 + ((i128)nb - 1) * step;   // nb == 0: one step before t0, no bucket
  const i128 times[] = {(i128)t0 - 1, t0, (i128)t0 + 1, (i128)t0 + step - 1, (i128)t0 + step, last - 1, last, last + 1, last + step - 1, last + step,
                        (i128)t0 + 0xFFFFFFFFll, (i128)t0 + 0x100000000ll, (i128)t0 + 0x100000000ll - step, (i128)t0 + 0x100000000ll + step, kMin, kMin + 1,
                        kMax - 1, kMax, 0, -1, 1};
  for (i128 t : times) check_time(L, t);
}

static void lattices() {
  const int64_t t0s[] = {0, 1, 1700000000, -1, -1700000000, -86400 * 365 * 1000ll, INT64_MIN, INT64_MIN + 7};
  for (int64_t t0 : t0s) {
    for (uint64_t nb : {0ull, 1ull, 2ull, 120ull}) {
      check_lattice(t0, 1, nb, 0);
      check_lattice(t0, 60, nb, 1);
      check_lattice(t0, 65539, nb, 1);
      check_lattice(t0, 1ll << 32, nb, 2);                       // a step of 2^32 or more is never a multiply-high
      check_lattice(t0, (1ll << 33) + 1, nb, 2);
    }
    // a span of exactly 2^32 - 1 (the last dividend the multiply-high is exact for), and of 2^32
    check_lattice(t0, 1, 1ull << 32, 0);                           // span 2^32 - 1
    check_lattice(t0, 1, (1ull << 32) + 1, 0);                     // span 2^32
    check_lattice(t0, 3, 1431655766ull, 1);                        // 3 * 1431655765 = 2^32 - 1
    check_lattice(t0, 65537, 65536ull, 1);                         // 65537 * 65535 = 2^32 - 1
    check_lattice(t0, 2, (1ull << 31) + 1, 2);                     // 2 * 2^31 = 2^32: division
    check_lattice(t0, 65536, 65537ull, 2);                         // 65536 * 65536 = 2^32
    check_lattice(t0, 65538, 65535ull, 1);                         // last bucket at 2^32 - 4
    check_lattice(t0, 65538, 65537ull, 2);
  }
  // up to the last time there is
  check_lattice(INT64_MAX, 1, 1, 0);
  check_lattice(INT64_MAX - 119, 1, 120, 0);
  check_lattice(INT64_MAX - 60 * 119, 60, 120, 1);
  check_lattice(INT64_MAX - ((1ll << 33) + 1) * 119, (1ll << 33) + 1, 120, 2);
  check_lattice(INT64_MIN, 1ll << 62, 4, 2);                       // INT64_MIN .. INT64_MIN + 3 * 2^62: the whole range in four buckets
  check_lattice(INT64_MIN, INT64_MAX, 3, 2);
  CHECK(make_lattice(5, 0, 3).step == 1 && make_lattice(5, -7, 3).step == 1);   // a step below 1 is 1
  CHECK(n_bucket[0] > 0 && n_bucket[1] > 0 && n_bucket[2] > 0);
}

static void window() {
  const int64_t S = 1700000000, E = 1700003600;
  for (int64_t te : {E - 1, E}) {
    for (int64_t ts : {S - 1, S}) {
      const bool in_end = te < E, in_start = ts >= S;
      CHECK(time_kept(te, ts, true, RowFilter{S, E}) == (in_end && in_start));
      CHECK(time_kept(te, ts, false, RowFilter{S, E}) == in_end);          // no start column: start_time judges nothing
      CHECK(time_kept(te, ts, true, RowFilter{0, E}) == in_end);           // 0 = unset
      CHECK(time_kept(te, ts, false, RowFilter{0, E}) == in_end);
      CHECK(time_kept(te, ts, true, RowFilter{S, 0}) == in_start);
      CHECK(time_kept(te, ts, false, RowFilter{S, 0}));
      CHECK(time_kept(te, ts, true, RowFilter{0, 0}) && time_kept(te, ts, false, RowFilter{0, 0}));
    }
  }
  CHECK(!time_kept(INT64_MAX, INT64_MIN, true, RowFilter{S, E}) && time_kept(INT64_MIN, INT64_MAX, true, RowFilter{S, E}));
}

static uint64_t rnd_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull; return rnd_state >> 17; }

// merge times[lo, hi) as a random binary tree of accumulators; now and then an empty accumulator joins on either side
static LatticeAcc merge_range(const std::vector<int64_t> &t, size_t lo, size_t hi) {
  const LatticeAcc none{0, 0, 0, 0, 0};
  LatticeAcc a;
  if (hi - lo == 1) {
    a = LatticeAcc{t[lo], t[lo], t[lo], 0, 1};
  } else {
    const size_t mid = lo + 1 + (size_t)(rnd() % (hi - lo - 1));
    a = lattice_merge(merge_range(t, lo, mid), merge_range(t, mid, hi));
    ++n_merge;
  }
  switch (rnd() % 4) {
    case 0: return lattice_merge(none, a);
    case 1: return lattice_merge(a, none);
    default: return a;
  }
}

static void merges() {
  const int64_t t0s[] = {0, 1700000000, -1700000000, INT64_MIN, INT64_MAX - 1000ll * 4096};
  const int64_t steps[] = {1, 60, 4096, 1ll << 40};
  for (int64_t t0 : t0s)
    for (int64_t step : steps)
      for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)17, (size_t)200}) {
        const uint64_t nb = step == (1ll << 40) ? (t0 == INT64_MAX - 1000ll * 4096 ? 1 : 1000) : 1000;
        std::vector<int64_t> t(n);
        for (size_t i = 0; i < n; ++i) t[i] = (int64_t)((i128)t0 + (i128)(rnd() % nb) * step);
        int64_t tmin = t[0], tmax = t[0];
        for (int64_t x : t) { tmin = x < tmin ? x : tmin; tmax = x > tmax ? x : tmax; }
        for (int round = 0; round < 8; ++round) {
          const LatticeAcc a = merge_range(t, 0, n);
          CHECK(a.used == n && a.tmin == tmin && a.tmax == tmax);
          bool differ = false;
          for (int64_t x : t) {
            const uint64_t d = absdiff_i64(x, a.tref);
            differ |= d != 0;
            CHECK(d == 0 || (a.g != 0 && d % a.g == 0));     // g divides every difference to the reference time ...
            CHECK(absdiff_i64(x, tmin) == 0 || (a.g != 0 && absdiff_i64(x, tmin) % a.g == 0));   // ... and so every difference there is
          }
          CHECK(differ == (a.g != 0));
          CHECK(a.g % (uint64_t)step == 0);                  // and is no finer than the lattice the times came from
        }
      }
  CHECK(n_merge > 1000);
  CHECK(gcd_u64(0, 0) == 0 && gcd_u64(0, 9) == 9 && gcd_u64(9, 0) == 9 && gcd_u64(12, 18) == 6);
  CHECK(gcd_u64(3ull << 40, 9ull << 33) == 3ull << 33 && gcd_u64(UINT64_MAX, UINT64_MAX - 1) == 1);
  CHECK(absdiff_i64(INT64_MIN, INT64_MAX) == UINT64_MAX && absdiff_i64(INT64_MAX, INT64_MIN) == UINT64_MAX && absdiff_i64(-3, -3) == 0);
}

static void key_slots() {
  const uint64_t Ks[] = {1, 2, 3000, 1ull << 32, UINT64_MAX - 1};
  for (uint64_t K : Ks) {
    uint32_t err = 0;
    CHECK(key_slot(true, kKeySkip, K, err) == kSlotSkip && err == 0);
    CHECK(key_slot(true, 0, K, err) == kSlotLive && err == 0);
    CHECK(key_slot(true, K - 1, K, err) == kSlotLive && err == 0);
    CHECK(key_slot(false, K, K, err) == kSlotSkip && err == 0);             // a row outside the time window raises nothing
    CHECK(key_slot(false, K - 1, K, err) == kSlotSkip && err == 0);
    CHECK(key_slot(true, K, K, err) == kSlotRange && err == DEV_ERR_KEY_RANGE);
    err = DEV_ERR_OFF_LATTICE;
    CHECK(key_slot(true, UINT64_MAX - 1, K, err) == kSlotRange && err == (DEV_ERR_OFF_LATTICE | DEV_ERR_KEY_RANGE));   // 2^64 - 2, the last id that is not the skip key; bits are added, never cleared
  }
  uint32_t err = 0;
  CHECK(key_slot(true, 0, 0, err) == kSlotRange && err == DEV_ERR_KEY_RANGE);   // no keys at all
}

static void columns() {
  alignas(16) static uint64_t buf[8];
  RowCols r{buf, nullptr, reinterpret_cast<const int64_t *>(buf + 2), nullptr, buf + 4, 4, 0};
  CHECK(!r.has2() && r.keys_aligned16() && r.aligned16() && r.start_aligned16());
  r.key2 = buf + 1;
  CHECK(r.has2() && !r.keys_aligned16() && !r.aligned16());
  r.key2 = buf + 6; r.value = buf + 5;
  CHECK(r.keys_aligned16() && !r.aligned16());
  r.t_start = reinterpret_cast<const int64_t *>(buf + 7);
  CHECK(!r.start_aligned16());
}

int main() {
  lattices();
  window();
  merges();
  key_slots();
  columns();
  printf("bucket checks %ld %ld %ld fast %ld merges %ld\n", n_bucket[0], n_bucket[1], n_bucket[2], n_fast, n_merge);
  return 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_row_judges_against_128_bit_arithmetic(tmp_path, sanitize):
    src = tmp_path / "row_judge.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "row_judge"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bucket checks" in r.stdout and r.stderr == "", r.stdout + r.stderr
