"""The workspace layouts (theia_amd/csrc/tad_carve.h) checked on the host: a stand-alone g++ program includes the header alone and, for
every layout over a sweep of small dimensions, checks that the measuring walk and the placing walk end at the same byte count, that the
count is the formula the host code used before the header existed, that every pointer is the one the old pointer chain formed (both written
out literally below), that no array touches another, a guard or the outside, and that no array starts off its alignment.  No GPU, no
library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tad_carve.h"
using namespace tad;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

typedef unsigned char u8;
typedef unsigned long long u64;
struct Part { const void *p; size_t bytes; };
typedef std::vector<Part> Parts;
#define PART(v, ptr, n) (v).push_back(Part{(ptr), (size_t)(n) * sizeof(*(ptr))})
#define PARTB(v, ptr, bytes) (v).push_back(Part{(ptr), (size_t)(bytes)})

static long blocks = 0, arrays = 0;
constexpr size_t kGuard = 64;

// walk(c, parts, base): runs the layout over the walkers c[0 .. N), lists every array of block i in parts[i] and, when base[i] != NULL,
// compares the pointers with the old chain.  want[i]: the old size formula of block i
template <size_t N, typename F> static void check(const size_t (&want)[N], F walk) {
  Parts parts[N];
  u8 *none[N] = {};
  {   // measure: no base, no pointer
    Carve m[N] = {Carve(nullptr), Carve(nullptr)};
    walk(m, parts, none);
    for (size_t i = 0; i < N; ++i) {
      CHECK(m[i].bytes() == want[i]);
      CHECK(!m[i].misaligned());
      for (const Part &p : parts[i]) CHECK(p.p == nullptr || p.bytes == 0);
      parts[i].clear();
    }
  }
  u8 *raw[N], *base[N];
  for (size_t i = 0; i < N; ++i) {
    const size_t all = (want[i] + 2 * kGuard + 255) / 256 * 256;
    raw[i] = static_cast<u8 *>(aligned_alloc(256, all + 256));
    CHECK(raw[i] != nullptr);
    memset(raw[i], 0xEE, all + 256);
    base[i] = raw[i] + 256;              // 256-byte aligned like a device allocation, a guard on either side
  }
  Carve c[N] = {Carve(base[0]), Carve(N > 1 ? base[1] : nullptr)};
  walk(c, parts, base);
  for (size_t i = 0; i < N; ++i) {
    CHECK(c[i].bytes() == want[i]);      // measure == place == the old formula
    CHECK(!c[i].misaligned());
    ++blocks;
    for (const Part &p : parts[i]) {     // inside the block, before anything is written
      if (p.bytes == 0) continue;
      const u8 *b = static_cast<const u8 *>(p.p);
      CHECK(b >= base[i] && b + p.bytes <= base[i] + want[i]);
    }
    for (size_t k = 0; k < parts[i].size(); ++k) memset(const_cast<void *>(parts[i][k].p), (int)(k + 1), parts[i][k].bytes);
    for (size_t k = 0; k < parts[i].size(); ++k) {
      const u8 *b = static_cast<const u8 *>(parts[i][k].p);
      for (size_t j = 0; j < parts[i][k].bytes; ++j) CHECK(b[j] == (u8)(k + 1));   // no later array wrote into this one
      ++arrays;
    }
    for (size_t j = 0; j < kGuard; ++j) CHECK(base[i][-(long)j - 1] == 0xEE && base[i][want[i] + j] == 0xEE);
    free(raw[i]);
  }
}
template <typename F> static void check1(size_t want, F walk) {
  const size_t w[2] = {want, 0};
  check(w, [&](Carve *c, Parts *parts, u8 **base) { walk(c[0], parts[0], base[0]); });
}

static void state_parts(Parts &v, const StreamState &s, uint64_t K) {
  PART(v, s.avg, K); PART(v, s.m2, K); PART(v, s.ewma, K); PART(v, s.last_t, K); PART(v, s.n, K); PART(v, s.seen, K);
}
// the old stream_view
static void state_chain(const StreamState &v, u8 *b, uint64_t K) {
  CHECK(v.avg == reinterpret_cast<double *>(b));
  CHECK(v.m2 == v.avg + K);
  CHECK(v.ewma == v.m2 + K);
  CHECK(v.last_t == reinterpret_cast<long long *>(v.ewma + K));
  CHECK(v.n == reinterpret_cast<uint32_t *>(v.last_t + K));
  CHECK(v.seen == reinterpret_cast<unsigned char *>(v.n + K));
}

static void per_key(uint64_t K) {
  const size_t kpad = (size_t)((K + 3) & ~3ull), ko = kpad + 4;
  CHECK(sizeof(MergeCounters) == 64 && sizeof(CompactCounters) == 64);
  // a state's block: state_bytes / stream_view
  check1((size_t)K * (4 + 8 * 4 + 1) + 64, [&](Carve &c, Parts &v, u8 *b) {
    const StreamState s = stream_state_layout(c, K);
    state_parts(v, s, K);
    if (b) state_chain(s, b, K);
  });
  {   // ensure_batch_points / stream_history_batch
    const size_t want[2] = {(kpad + 4) * 16, kpad * 4 + 64};   // (hs_koff, then hs_kcnt)
    check(want, [&](Carve *c, Parts *v, u8 **b) {
      const BatchKeys k = batch_keys_layout(c[0], c[1], K);
      PART(v[1], k.kcnt, kpad); PART(v[1], k.long_count, 1); PART(v[0], k.koff, ko); PART(v[0], k.coff, ko);
      if (!b[0]) return;
      unsigned long long *koff = reinterpret_cast<unsigned long long *>(b[0]), *coff = koff + kpad + 4;
      uint32_t *kcnt = reinterpret_cast<uint32_t *>(b[1]);
      unsigned int *long_count = reinterpret_cast<unsigned int *>(kcnt + kpad);
      CHECK(k.kcnt == kcnt && k.long_count == long_count && k.koff == koff && k.coff == coff);
    });
  }
  {   // tad_state_trim
    const size_t want[2] = {kpad * 12 + 64, (kpad + 4) * 16};
    check(want, [&](Carve *c, Parts *v, u8 **b) {
      const TrimKeys k = trim_keys_layout(c[0], c[1], K);
      PART(v[0], k.rcnt, kpad); PART(v[0], k.ecnt, kpad); PART(v[0], k.chunks, kpad); PART(v[0], k.long_count, 1);
      PART(v[1], k.eoff, ko); PART(v[1], k.coff, ko);
      if (!b[0]) return;
      uint32_t *rcnt = reinterpret_cast<uint32_t *>(b[0]), *ecnt = rcnt + kpad, *chunks = ecnt + kpad;
      unsigned int *long_count = reinterpret_cast<unsigned int *>(chunks + kpad);
      unsigned long long *eoff = reinterpret_cast<unsigned long long *>(b[1]), *coff = eoff + kpad + 4;
      CHECK(k.rcnt == rcnt && k.ecnt == ecnt && k.chunks == chunks && k.long_count == long_count && k.eoff == eoff && k.coff == coff);
    });
  }
  {   // tad_state_compact, and its summed need with a host and a device remap
    const size_t cnt_bytes = kpad * 20 + 64, off_bytes = (kpad + 4) * 40;
    const size_t want[2] = {cnt_bytes, off_bytes};
    check(want, [&](Carve *c, Parts *v, u8 **b) {
      const CompactKeys k = compact_keys_layout(c[0], c[1], K);
      PART(v[0], k.live, kpad); PART(v[0], k.slen, kpad); PART(v[0], k.hlen, kpad); PART(v[0], k.schunks, kpad); PART(v[0], k.hchunks, kpad);
      PART(v[0], k.cc, 1);
      PART(v[1], k.newid, ko); PART(v[1], k.sscan, ko); PART(v[1], k.hscan, ko); PART(v[1], k.scoff, ko); PART(v[1], k.hcoff, ko);
      if (!b[0]) return;
      uint32_t *live = reinterpret_cast<uint32_t *>(b[0]), *slen = live + kpad, *hlen = slen + kpad, *schunks = hlen + kpad, *hchunks = schunks + kpad;
      CompactCounters *cc = reinterpret_cast<CompactCounters *>(hchunks + kpad);
      unsigned long long *newid = reinterpret_cast<unsigned long long *>(b[1]), *sscan = newid + kpad + 4, *hscan = sscan + kpad + 4,
                         *scoff = hscan + kpad + 4, *hcoff = scoff + kpad + 4;
      CHECK(k.live == live && k.slen == slen && k.hlen == hlen && k.schunks == schunks && k.hchunks == hchunks && k.cc == cc);
      CHECK(k.newid == newid && k.sscan == sscan && k.hscan == hscan && k.scoff == scoff && k.hcoff == hcoff);
    });
    for (int host_remap = 0; host_remap < 2; ++host_remap)
      for (size_t scan_bytes : {(size_t)16, (size_t)(((K + 1023) / 1024 + 1) * 8)})
        CHECK(compact_workspace_bytes(K, scan_bytes, host_remap != 0) == cnt_bytes + off_bytes + scan_bytes + (host_remap ? (size_t)K * 8 : 0));
  }
  // view_detect, and tad_drop_stream's touched keys (run_job_locked cut them as hs_kcnt and hs_kcnt + ((K + 3) & ~3ull))
  check1(kpad * 4 + 64, [&](Carve &c, Parts &v, u8 *b) {
    const ViewRoute r = view_route_layout(c, K);
    PART(v, r.list, kpad); PART(v, r.lcount, 1);
    if (!b) return;
    uint32_t *list = reinterpret_cast<uint32_t *>(b);
    CHECK(r.list == list && r.lcount == reinterpret_cast<unsigned int *>(list + kpad));
    CHECK(r.lcount == reinterpret_cast<unsigned int *>(reinterpret_cast<uint32_t *>(b) + ((K + 3) & ~3ull)));
  });
  // window_bounds: win_key_bytes(K) + state_bytes(K), win_keys
  check1(kpad * 16 + 64 + (kpad + 4) * 24 + (size_t)K * (4 + 8 * 4 + 1) + 64, [&](Carve &c, Parts &v, u8 *b) {
    const WinKeys k = win_keys_layout(c, K);
    PART(v, k.wbeg, kpad); PART(v, k.wlen, kpad); PART(v, k.ecnt, kpad); PART(v, k.chunks, kpad); PART(v, k.long_count, 1);
    PART(v, k.woff, ko); PART(v, k.coff, ko); PART(v, k.eoff, ko);
    state_parts(v, k.wmom, K);
    if (!b) return;
    WinKeys w;
    w.wbeg = reinterpret_cast<uint32_t *>(b); w.wlen = w.wbeg + kpad; w.ecnt = w.wlen + kpad; w.chunks = w.ecnt + kpad;
    w.long_count = reinterpret_cast<unsigned int *>(w.chunks + kpad);
    w.woff = reinterpret_cast<unsigned long long *>(reinterpret_cast<unsigned char *>(w.long_count) + 64);
    w.coff = w.woff + kpad + 4; w.eoff = w.coff + kpad + 4;
    CHECK(k.wbeg == w.wbeg && k.wlen == w.wlen && k.ecnt == w.ecnt && k.chunks == w.chunks && k.long_count == w.long_count);
    CHECK(k.woff == w.woff && k.coff == w.coff && k.eoff == w.eoff);
    state_chain(k.wmom, b + (kpad * 16 + 64 + (kpad + 4) * 24), K);
  });
  // state_merge_batch: mg_keys
  check1(128 + ko * 40 + kpad * 16, [&](Carve &c, Parts &v, u8 *b) {
    const MergeKeys k = merge_keys_layout(c, K);
    PART(v, k.mcnt, 1); PART(v, k.long_count, 1);
    PART(v, k.akoff, ko); PART(v, k.rkoff, ko); PART(v, k.hoff_mid, ko); PART(v, k.coff_s, ko); PART(v, k.coff_h, ko);
    PART(v, k.chunks_s, kpad); PART(v, k.chunks_h, kpad); PART(v, k.replay, kpad); PART(v, k.long_list, kpad);
    if (!b) return;
    MergeCounters *mcnt = reinterpret_cast<MergeCounters *>(b);
    unsigned int *long_count = reinterpret_cast<unsigned int *>(mcnt + 1);
    unsigned long long *akoff = reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(b) + 128), *rkoff = akoff + ko;
    unsigned long long *hoff_mid = rkoff + ko, *coff_s = hoff_mid + ko, *coff_h = coff_s + ko;
    uint32_t *chunks_s = reinterpret_cast<uint32_t *>(coff_h + ko), *chunks_h = chunks_s + kpad, *replay = chunks_h + kpad, *long_list = replay + kpad;
    CHECK(k.mcnt == mcnt && k.long_count == long_count && k.akoff == akoff && k.rkoff == rkoff && k.hoff_mid == hoff_mid && k.coff_s == coff_s);
    CHECK(k.coff_h == coff_h && k.chunks_s == chunks_s && k.chunks_h == chunks_h && k.replay == replay && k.long_list == long_list);
  });
  // stream_arima_batch: as_key
  check1(kpad * 8 + (kpad + 4) * 16 + 64 + kpad * (4 * 3 + 1 + 8 * 4) + 256, [&](Carve &c, Parts &v, u8 *b) {
    const ArimaKeys k = arima_keys_layout(c, K);
    PART(v, k.touched, kpad); PART(v, k.len8, kpad); PART(v, k.tidx, ko); PART(v, k.yoffk, ko); PART(v, k.tmax, 1);
    PART(v, k.sl.yoff, kpad); PART(v, k.sl.lam, kpad); PART(v, k.sl.sigma, kpad); PART(v, k.sl.ibase, kpad);
    PART(v, k.sl.key, kpad); PART(v, k.sl.lo, kpad); PART(v, k.sl.hi, kpad); PART(v, k.sl.ok, kpad);
    if (!b) return;
    unsigned char *kb = b;
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
    CHECK(k.touched == touched && k.len8 == len8 && k.tidx == tidx && k.yoffk == yoffk && k.tmax == tmax_dev);
    CHECK(k.sl.yoff == sl.yoff && k.sl.lam == sl.lam && k.sl.sigma == sl.sigma && k.sl.ibase == sl.ibase);
    CHECK(k.sl.key == sl.key && k.sl.lo == sl.lo && k.sl.hi == sl.hi && k.sl.ok == sl.ok);
  });
  {   // state_drop_batch: drop_state_key_bytes / drop_state_keys (kpad rounds to 8 here)
    const size_t kpad8 = (size_t)((K + 7) & ~7ull);
    check1(kpad8 * (3 * sizeof(double) + sizeof(uint32_t) + 1) + 64, [&](Carve &c, Parts &v, u8 *b) {
      const DropStateKeys k = drop_state_keys_layout(c, K);
      PART(v, k.mean, kpad8); PART(v, k.std, kpad8); PART(v, k.m2, kpad8); PART(v, k.n, kpad8); PART(v, k.ok, kpad8);
      if (!b) return;
      DropStateKeys d;
      d.mean = reinterpret_cast<double *>(b);
      d.std = d.mean + kpad8;
      d.m2 = d.std + kpad8;
      d.n = reinterpret_cast<uint32_t *>(d.m2 + kpad8);
      d.ok = reinterpret_cast<uint8_t *>(d.n + kpad8);
      CHECK(k.mean == d.mean && k.std == d.std && k.m2 == d.m2 && k.n == d.n && k.ok == d.ok);
    });
  }
  // sparse_stream_offsets: sp_cls
  check1(kpad * 4 + (K + 1) * 8 + 64, [&](Carve &c, Parts &v, u8 *b) {
    const StreamPoints p = stream_points_layout(c, K);
    PART(v, p.len, kpad); PART(v, p.poff, K + 1);
    if (!b) return;
    uint32_t *len = reinterpret_cast<uint32_t *>(b);
    CHECK(p.len == len && p.poff == reinterpret_cast<unsigned long long *>(len + kpad));
  });
  // run_sparse_classes: sp_cls
  check1(kpad * 12 + (kpad + 4) * 16 + 64, [&](Carve &c, Parts &v, u8 *b) {
    const ClassKeys k = class_keys_layout(c, K);
    PART(v, k.len, kpad); PART(v, k.member, kpad); PART(v, k.pts, kpad); PART(v, k.key_off, ko); PART(v, k.pt_off, ko);
    if (!b) return;
    uint32_t *len = reinterpret_cast<uint32_t *>(b), *member = len + kpad, *pts = member + kpad;
    unsigned long long *key_off = reinterpret_cast<unsigned long long *>(pts + kpad), *pt_off = key_off + kpad + 4;
    CHECK(k.len == len && k.member == member && k.pts == pts && k.key_off == key_off && k.pt_off == pt_off);
  });
}

static void per_point(uint64_t P_cap) {
  const uint64_t pc = P_cap ? P_cap : 1;   // (both callers map 0 to 1)
  // state_merge_batch: mg_pts
  check1((7 * pc + 8) * 8 + pc * 16 + pc + 64, [&](Carve &c, Parts &v, u8 *b) {
    const MergePts m = merge_pts_layout(c, pc);
    PART(v, m.nhoff, pc + 2); PART(v, m.aoff, pc + 2); PART(v, m.roff, pc + 2);
    PART(v, m.hadd, pc); PART(v, m.hadd_s, pc); PART(v, m.hrem, pc); PART(v, m.hrem_s, pc);
    PART(v, m.rank, pc); PART(v, m.f_nh, pc); PART(v, m.f_kept, pc); PART(v, m.f_hit, pc); PART(v, m.cls, pc);
    if (!b) return;
    unsigned long long *nhoff = reinterpret_cast<unsigned long long *>(b), *aoff = nhoff + pc + 2, *roff = aoff + pc + 2;
    unsigned long long *hadd = roff + pc + 2, *hadd_s = hadd + pc, *hrem = hadd_s + pc, *hrem_s = hrem + pc;
    uint32_t *rank = reinterpret_cast<uint32_t *>(hrem_s + pc), *f_nh = rank + pc, *f_kept = f_nh + pc, *f_hit = f_kept + pc;
    uint8_t *cls = reinterpret_cast<uint8_t *>(f_hit + pc);
    CHECK(m.nhoff == nhoff && m.aoff == aoff && m.roff == roff && m.hadd == hadd && m.hadd_s == hadd_s && m.hrem == hrem && m.hrem_s == hrem_s);
    CHECK(m.rank == rank && m.f_nh == f_nh && m.f_kept == f_kept && m.f_hit == f_hit && m.cls == cls);
  });
  // state_drop_batch: ds_pt
  check1((pc + 1) * 8 + pc * 4 + pc + 64, [&](Carve &c, Parts &v, u8 *b) {
    const DropPts d = drop_pts_layout(c, pc);
    PART(v, d.row, pc + 1); PART(v, d.cnt, pc); PART(v, d.flag, pc);
    if (!b) return;
    unsigned long long *row = reinterpret_cast<unsigned long long *>(b);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(row + pc + 1);
    uint8_t *flag = reinterpret_cast<uint8_t *>(cnt + pc);
    CHECK(d.row == row && d.cnt == cnt && d.flag == flag);
  });
  if (P_cap == 0) return;   // the blocks below are only built for P >= 1
  const uint64_t P = P_cap;
  // stream_arima_batch: as_pt
  const size_t ppad = (size_t)((P + 3) & ~3ull);
  check1(ppad * (8 + 4 + 8 + 1) + 64, [&](Carve &c, Parts &v, u8 *b) {
    const ArimaPts a = arima_pts_layout(c, P);
    PART(v, a.pcalc, ppad); PART(v, a.rows, ppad); PART(v, a.row_off, ppad + 4); PART(v, a.pflag, ppad);
    if (!b) return;
    double *pcalc = reinterpret_cast<double *>(b);
    uint32_t *rows = reinterpret_cast<uint32_t *>(pcalc + ppad);
    unsigned long long *row_off = reinterpret_cast<unsigned long long *>(rows + ppad);
    uint8_t *pflag = reinterpret_cast<uint8_t *>(row_off + ppad + 4);
    CHECK(a.pcalc == pcalc && a.rows == rows && a.row_off == row_off && a.pflag == pflag);
  });
  // window_gather: wv_pts
  for (int dbscan = 0; dbscan < 2; ++dbscan)
    check1(P * (dbscan ? 24 : 16), [&](Carve &c, Parts &v, u8 *b) {
      const WinPts w = win_pts_layout(c, P, dbscan != 0);
      PART(v, w.wval, P); PART(v, w.wt, P);
      if (dbscan) PART(v, w.wh, P);
      CHECK(dbscan || w.wh == nullptr);
      if (!b) return;
      unsigned long long *wval = reinterpret_cast<unsigned long long *>(b);
      long long *wt = reinterpret_cast<long long *>(wval + P);
      unsigned long long *wh = wval + 2 * P;
      CHECK(w.wval == wval && w.wt == wt && (!dbscan || w.wh == wh));
    });
  // run_sparse_classes: the class tables
  for (uint64_t K : {(uint64_t)1, (uint64_t)3, P, P + 5}) {
    const uint64_t kmax = K < P ? K : P;
    check1((size_t)P * 24 + (size_t)kmax * 4 + 256, [&](Carve &c, Parts &v, u8 *b) {
      const ClassTables t = class_tables_layout(c, P, kmax);
      PART(v, t.key, P); PART(v, t.t, P); PART(v, t.val, P); PART(v, t.map, kmax);
      if (!b) return;
      unsigned long long *c_key = reinterpret_cast<unsigned long long *>(b);
      long long *c_t = reinterpret_cast<long long *>(c_key + P);
      unsigned long long *c_val = reinterpret_cast<unsigned long long *>(c_t + P);
      uint32_t *c_map = reinterpret_cast<uint32_t *>(c_val + P);
      CHECK(t.key == c_key && t.t == c_t && t.val == c_val && t.map == c_map);
    });
  }
}

static void results() {
  for (uint64_t rows : {0, 1, 3, 4, 5, 15, 16, 17})
    for (int with_anomaly = 0; with_anomaly < 2; ++with_anomaly) {
      const uint64_t r = ((rows ? rows : 1) + 3) & ~3ull;
      check1((size_t)r * 8 * 5 + (with_anomaly ? (size_t)((r + 15) & ~15ull) : 0), [&](Carve &c, Parts &v, u8 *b) {
        const OutRows o = result_layout(c, rows, with_anomaly != 0);
        PART(v, o.key_id, r); PART(v, o.flow_end_s, r); PART(v, o.throughput, r); PART(v, o.algo_calc, r); PART(v, o.stddev, r);
        if (with_anomaly) PART(v, o.anomaly, (r + 15) & ~15ull);
        CHECK(with_anomaly || o.anomaly == nullptr);
        if (!b) return;
        unsigned char *p = b;
        CHECK(o.key_id == reinterpret_cast<unsigned long long *>(p)); p += r * 8;
        CHECK(o.flow_end_s == reinterpret_cast<long long *>(p)); p += r * 8;
        CHECK(o.throughput == reinterpret_cast<double *>(p)); p += r * 8;
        CHECK(o.algo_calc == reinterpret_cast<double *>(p)); p += r * 8;
        CHECK(o.stddev == reinterpret_cast<double *>(p)); p += r * 8;
        CHECK(o.anomaly == (with_anomaly ? p : nullptr));
      });
    }
  for (uint64_t m : {1, 3, 4, 5}) {   // tad_drop_select's rows
    const uint64_t stride = (m + 3) & ~3ull;
    check1((size_t)stride * 8 * 7, [&](Carve &c, Parts &v, u8 *d) {
      const DselOut o = drop_rows_layout(c, m);
      PART(v, o.kind, stride); PART(v, o.ns, stride); PART(v, o.name, stride); PART(v, o.dir, stride); PART(v, o.day, stride);
      PART(v, o.count, stride); PART(v, o.row, stride);
      if (!d) return;
      CHECK(o.kind == reinterpret_cast<long long *>(d) && o.ns == reinterpret_cast<long long *>(d + stride * 8));
      CHECK(o.name == reinterpret_cast<long long *>(d + stride * 16) && o.dir == reinterpret_cast<long long *>(d + stride * 24));
      CHECK(o.day == reinterpret_cast<long long *>(d + stride * 32) && o.count == reinterpret_cast<unsigned long long *>(d + stride * 40));
      CHECK(o.row == reinterpret_cast<unsigned long long *>(d + stride * 48));
    });
  }
}

static void arima() {
  for (uint64_t npos : {1, 2, 15, 16, 17})   // as_pos
    check1(npos * (4 + 8) + 128, [&](Carve &c, Parts &v, u8 *b) {
      const ArimaPos a = arima_pos_layout(c, npos);
      PART(v, a.pcnt, npos); PART(v, a.loff, npos + 1);
      if (!b) return;
      CHECK(a.pcnt == reinterpret_cast<unsigned int *>(b));
      CHECK(a.loff == reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(b) + ((npos * 4 + 63) & ~63ull)));
      CHECK((reinterpret_cast<uintptr_t>(a.loff) & 63) == 0);
    });
  for (uint64_t nfits : {0, 1, 3, 4, 5})     // as_fit
    for (uint64_t waves : {0, 1, 5}) {
      const size_t fpad = (size_t)((nfits + 3) & ~3ull);
      check1(fpad * 8 + (size_t)(waves + 4) * 4 + 64, [&](Carve &c, Parts &v, u8 *b) {
        const ArimaFits a = arima_fits_layout(c, nfits, waves);
        PART(v, a.list, fpad); PART(v, a.fpos, fpad); PART(v, a.wpos, waves + 4);
        if (!b) return;
        uint32_t *list = reinterpret_cast<uint32_t *>(b), *fpos = list + fpad, *wpos = fpos + fpad;
        CHECK(a.list == list && a.fpos == fpos && a.wpos == wpos);
      });
    }
  const uint64_t s8_tmax[2][2] = {{8, 1}, {64, 17}};   // as_ser
  for (const auto &d : s8_tmax) {
    const uint64_t S8 = d[0];
    const unsigned int tmax = (unsigned int)d[1];
    const size_t ser = (size_t)S8 + tmax + 32;
    check1(ser * 16, [&](Carve &c, Parts &v, u8 *b) {
      const ArimaSeries a = arima_series_layout(c, S8, tmax);
      CHECK(a.ser == ser);
      PART(v, a.lx, S8 + tmax); PART(v, a.ysk, a.ser);   // (ysk is zeroed over its slack too)
      if (!b) return;
      double *lx = reinterpret_cast<double *>(b), *ysk = lx + ser;
      CHECK(a.lx == lx && a.ysk == ysk);
    });
  }
  for (size_t tb : {(size_t)256, (size_t)512, (size_t)4096})   // sparse_sort: sp_temp (tb: sparse_sort_temp_bytes, a 256-byte multiple)
    check1(tb + 64, [&](Carve &c, Parts &v, u8 *b) {
      const SparseTemp t = sparse_temp_layout(c, tb);
      PARTB(v, t.temp, tb); PART(v, t.runs, 2);
      if (!b) return;
      CHECK(t.temp == b && t.runs == reinterpret_cast<unsigned long long *>(static_cast<unsigned char *>(b) + tb));
    });
}

static void dsel() {
  constexpr int kDselLaneRows = 16, kDselTileRows = 4096, kScanTile = 1024;
  for (uint64_t n : {1, 15, 16, 17, 4095, 4096, 4097})
    for (int t32 = 0; t32 < 2; ++t32)
      for (int mode = 0; mode < 5; ++mode) {   // a device table | a host table, with / without flow_end_s and keep
        const bool host = mode != 0, has_end = mode == 2 || mode == 4, has_keep = mode == 3 || mode == 4;
        const uint64_t tiles = (n + kDselTileRows - 1) / kDselTileRows;
        const size_t scan_elems = (size_t)((tiles + kScanTile - 1) / kScanTile) + 1;
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t bits_b = up((size_t)((n + kDselLaneRows - 1) / kDselLaneRows) * 2), cnt_b = up((size_t)tiles * 4), off_b = up((size_t)(tiles + 1) * 8);
        const size_t scr_b = up(scan_elems * 8), t_b = up((size_t)n * (t32 ? 4 : 8)), c_b = up((size_t)n * 8), a_b = up((size_t)n);
        const size_t stage = host ? 2 * a_b + t_b + (has_end ? t_b : 0) + 6 * c_b + (has_keep ? a_b : 0) : 0;
        const size_t need = bits_b + cnt_b + off_b + scr_b + 256 + stage;
        const DselDims dims{n, (n + kDselLaneRows - 1) / kDselLaneRows, tiles, scan_elems, t32 != 0, host, has_end, has_keep};
        check1(need, [&](Carve &c, Parts &v, u8 *b) {
          const DselWs w = dsel_layout(c, dims);
          const size_t tbytes = (size_t)n * (t32 ? 4 : 8);
          PART(v, w.bits, dims.words); PART(v, w.cnt, tiles); PART(v, w.off, tiles + 1); PART(v, w.scratch, scan_elems); PART(v, w.total, 1);
          if (host) {
            PART(v, w.ia, n); PART(v, w.ea, n); PARTB(v, w.ts, tbytes);
            if (has_end) PARTB(v, w.te, tbytes);
            for (int i = 0; i < 6; ++i) PART(v, w.codes[i], n);
            if (has_keep) PART(v, w.keep, n);
          }
          CHECK(host || (!w.ia && !w.ea && !w.ts && !w.codes[0] && !w.codes[5]));
          CHECK((has_end || !w.te) && (has_keep || !w.keep));
          if (!b) return;
          unsigned char *p = b;
          CHECK(w.bits == reinterpret_cast<uint16_t *>(p)); p += bits_b;
          CHECK(w.cnt == reinterpret_cast<uint32_t *>(p)); p += cnt_b;
          CHECK(w.off == reinterpret_cast<unsigned long long *>(p)); p += off_b;
          CHECK(w.scratch == reinterpret_cast<unsigned long long *>(p)); p += scr_b;
          CHECK(w.total == reinterpret_cast<unsigned long long *>(p)); p += 256;
          if (!host) return;
          CHECK(w.ia == p); p += a_b;      // the old put(): each column at p, then p += its room
          CHECK(w.ea == p); p += a_b;
          CHECK(w.ts == p); p += t_b;
          if (has_end) { CHECK(w.te == p); p += t_b; }
          for (int i = 0; i < 6; ++i) { CHECK(w.codes[i] == reinterpret_cast<long long *>(p)); p += c_b; }
          if (has_keep) { CHECK(w.keep == p); p += a_b; }
          CHECK(p == b + need);
        });
      }
}

int main() {
  {   // the walker itself: a take never pads, a start off its alignment sticks
    Carve c(nullptr);
    CHECK(c.take<uint8_t>(3) == nullptr && c.bytes() == 3 && !c.misaligned());
    c.take<uint32_t>(1);
    CHECK(c.bytes() == 7 && c.misaligned());
    c.pad(1);
    c.take<double>(1);
    CHECK(c.bytes() == 16 && c.misaligned());
    Carve d(nullptr);
    d.take<uint32_t>(4);
    d.take<double>(1, 16);
    CHECK(!d.misaligned() && d.pad_to(64) == 40 && d.pad_to(64) == 0 && d.bytes() == 64);
    d.take<uint32_t>(1);
    d.take<double>(1, 16);
    CHECK(d.misaligned());
  }
  for (uint64_t K : {1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025}) per_key(K);
  for (uint64_t P : {0, 1, 2, 3, 4, 5, 63, 64, 65}) per_point(P);
  results();
  arima();
  dsel();
  printf("blocks %ld arrays %ld\n", blocks, arrays);
  return 0;
}
"""


def test_every_layout_measures_what_it_places_and_places_what_the_old_chains_placed(tmp_path):
    src = tmp_path / "layout_walk.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout_walk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "blocks" in r.stdout, r.stdout
