// tad_carve.h — every workspace block that holds more than one array, described ONCE: a walker over a block (Carve) and, per block, a
// struct of typed pointers with the one function that walks it.  The same function measures the block (a walker without a base) and places
// its arrays (a walker over the allocated block), so a size and the pointers cut from it cannot drift apart.  Plain C++ (no HIP, no engine
// types): tests/test_workspace_layout.py checks every layout in a stand-alone program against the sizes and pointer chains it replaced.
//
// The rule: a take() never pads — an offset is what the takes and pads before it add up to.  Where a kernel loads an array 16 bytes at a
// time, or the code promised an alignment, the take names it and the walker's sticky flag records a start that misses it.  Slack is a
// pad() with its reason beside it; "unexplained, kept" marks slack whose reason nobody wrote down.
#ifndef THEIA_TAD_CARVE_H
#define THEIA_TAD_CARVE_H

#include <stddef.h>
#include <stdint.h>

namespace tad {

struct Carve {
  explicit Carve(void *base) : base_(static_cast<unsigned char *>(base)) {}   // NULL: measure only, no pointer is formed
  template <typename T> T *take(size_t n, size_t align = alignof(T)) {
    if (at_ % align != 0) misaligned_ = true;
    T *p = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
    at_ += n * sizeof(T);
    return p;
  }
  void pad(size_t bytes) { at_ += bytes; }
  size_t pad_to(size_t multiple) {   // up to the next multiple; returns the bytes it added
    const size_t add = (multiple - at_ % multiple) % multiple;
    at_ += add;
    return add;
  }
  size_t bytes() const { return at_; }            // where the walk stands = the block's size after the last take / pad
  bool misaligned() const { return misaligned_; }   // sticky: some take() began off its alignment

 private:
  unsigned char *base_;
  size_t at_ = 0;
  bool misaligned_ = false;
};

inline size_t kpad4(uint64_t K) { return (size_t)((K + 3) & ~3ull); }   // per-key u32 arrays: whole 16-byte groups
inline size_t kpad8(uint64_t K) { return (size_t)((K + 7) & ~7ull); }
// a per-key u32 array / an offset array of K + 1 entries (kpad + 4: the stride keeps the next array on 16 bytes)
inline uint32_t *take_counts(Carve &c, uint64_t K) { return c.take<uint32_t>(kpad4(K), 16); }
inline unsigned long long *take_offsets(Carve &c, uint64_t K) { return c.take<unsigned long long>(kpad4(K) + 4, 16); }
// one u32 in a 64-byte cell of its own (a list's length, a maximum: written by atomics, read back alone)
inline unsigned int *take_cell(Carve &c) {
  unsigned int *p = c.take<unsigned int>(1);
  c.pad(60);
  return p;
}

// ---- result blocks ----
struct OutRows {
  unsigned long long *key_id;
  long long *flow_end_s;
  double *throughput;
  double *algo_calc;
  double *stddev;
  uint8_t *anomaly;  // only with TAD_FLAG_EMIT_ALL_POINTS
};
// every column starts on a 32-byte boundary (stride = rows rounded up to 4): k_emit stores four rows at a time
inline OutRows result_layout(Carve &c, uint64_t rows, bool with_anomaly) {
  const size_t r = (size_t)(((rows ? rows : 1) + 3) & ~3ull);
  OutRows o;
  o.key_id = c.take<unsigned long long>(r, 32);
  o.flow_end_s = c.take<long long>(r, 32);
  o.throughput = c.take<double>(r, 32);
  o.algo_calc = c.take<double>(r, 32);
  o.stddev = c.take<double>(r, 32);
  o.anomaly = with_anomaly ? c.take<uint8_t>((r + 15) & ~(size_t)15, 32) : nullptr;
  return o;
}

// tad_drop_select's rows: seven columns of m values, each starting on a 32-byte boundary.  One layout for the emit kernel's arguments, the
// device block and its host copy
struct DselOut { long long *kind, *ns, *name, *dir, *day; unsigned long long *count, *row; };
inline DselOut drop_rows_layout(Carve &c, uint64_t m) {
  const size_t stride = (size_t)((m + 3) & ~3ull);
  DselOut o;
  o.kind = c.take<long long>(stride, 32);
  o.ns = c.take<long long>(stride, 32);
  o.name = c.take<long long>(stride, 32);
  o.dir = c.take<long long>(stride, 32);
  o.day = c.take<long long>(stride, 32);
  o.count = c.take<unsigned long long>(stride, 32);
  o.row = c.take<unsigned long long>(stride, 32);
  return o;
}

// ---- a streaming state's per-key block (tad_state::block[]), and the same arrays behind a window's view ----
struct StreamState {
  uint32_t *n;
  double *avg, *m2, *ewma;
  long long *last_t;
  unsigned char *seen;  // 0 until the key has seen a point
};
inline StreamState stream_state_layout(Carve &c, uint64_t K) {
  StreamState v;
  v.avg = c.take<double>(K);
  v.m2 = c.take<double>(K);
  v.ewma = c.take<double>(K);
  v.last_t = c.take<long long>(K);
  v.n = c.take<uint32_t>(K);
  v.seen = c.take<unsigned char>(K);
  c.pad(64);   // unexplained, kept
  return v;
}

// ---- hs_kcnt / hs_koff: per-key counts and offsets, one layout per use ----
// a batch on a history / series state (ensure_batch_points): dense point offsets | chunk offsets; counts (later the long-sort list /
// chunks) | long-list length.  (The offsets come first: this use has always grown hs_koff before hs_kcnt.)
struct BatchKeys {
  uint32_t *kcnt;
  unsigned int *long_count;
  unsigned long long *koff, *coff;
};
inline BatchKeys batch_keys_layout(Carve &off, Carve &cnt, uint64_t K) {
  BatchKeys b;
  b.koff = take_offsets(off, K);
  b.coff = take_offsets(off, K);
  b.kcnt = take_counts(cnt, K);
  b.long_count = take_cell(cnt);
  return b;
}
// tad_state_trim: retained | evicted | chunks (later the long-sort list) | its length; evicted offsets | chunk offsets
struct TrimKeys {
  uint32_t *rcnt, *ecnt, *chunks;
  unsigned int *long_count;
  unsigned long long *eoff, *coff;
};
inline TrimKeys trim_keys_layout(Carve &cnt, Carve &off, uint64_t K) {
  TrimKeys t;
  t.rcnt = take_counts(cnt, K);
  t.ecnt = take_counts(cnt, K);
  t.chunks = take_counts(cnt, K);
  t.long_count = take_cell(cnt);
  t.eoff = take_offsets(off, K);
  t.coff = take_offsets(off, K);
  return t;
}
// tad_state_compact: live | series lengths | history lengths | series chunks | history chunks | counters; new ids | candidate series
// offsets | candidate history offsets | series chunk offsets | history chunk offsets
struct CompactCounters {   // one 64-byte block on the device, zeroed per call
  unsigned long long unseen, idle, dropped, pad[5];   // keys with n == 0 | keys with last_t < retire_before | the points of those
};
struct CompactKeys {
  uint32_t *live, *slen, *hlen, *schunks, *hchunks;
  CompactCounters *cc;
  unsigned long long *newid, *sscan, *hscan, *scoff, *hcoff;
};
inline CompactKeys compact_keys_layout(Carve &cnt, Carve &off, uint64_t K) {
  CompactKeys k;
  k.live = take_counts(cnt, K);
  k.slen = take_counts(cnt, K);
  k.hlen = take_counts(cnt, K);
  k.schunks = take_counts(cnt, K);
  k.hchunks = take_counts(cnt, K);
  k.cc = cnt.take<CompactCounters>(1);
  k.newid = take_offsets(off, K);
  k.sscan = take_offsets(off, K);
  k.hscan = take_offsets(off, K);
  k.scoff = take_offsets(off, K);
  k.hcoff = take_offsets(off, K);
  return k;
}
// what tad_state_compact holds against the workspace limit: its two blocks, the scan scratch and a host remap's staging
inline size_t compact_workspace_bytes(uint64_t K, size_t scan_bytes, bool host_remap) {
  Carve cnt(nullptr), off(nullptr);
  compact_keys_layout(cnt, off, K);
  return cnt.bytes() + off.bytes() + scan_bytes + (host_remap ? (size_t)K * 8 : 0);
}
// a list of keys | its length: the long keys of a read-only job on a state (view_detect), the touched keys of tad_drop_stream
struct ViewRoute {
  uint32_t *list;
  unsigned int *lcount;
};
inline ViewRoute view_route_layout(Carve &c, uint64_t K) {
  ViewRoute r;
  r.list = take_counts(c, K);
  r.lcount = take_cell(c);
  return r;
}

// ---- tad_run_state_window's view (wv_key, wv_pts) ----
struct WinKeys {   // per key: window begin | window length | points outside | chunks (later the long-sort list) | the list's length | view offsets | chunk offsets | excluded offsets | moments
  uint32_t *wbeg, *wlen, *ecnt, *chunks;
  unsigned int *long_count;
  unsigned long long *woff, *coff, *eoff;
  StreamState wmom;
};
inline WinKeys win_keys_layout(Carve &c, uint64_t K) {
  WinKeys w;
  w.wbeg = take_counts(c, K);
  w.wlen = take_counts(c, K);
  w.ecnt = take_counts(c, K);
  w.chunks = take_counts(c, K);
  w.long_count = take_cell(c);
  w.woff = take_offsets(c, K);
  w.coff = take_offsets(c, K);
  w.eoff = take_offsets(c, K);
  w.wmom = stream_state_layout(c, K);
  return w;
}
struct WinPts {   // per window point: values | times | DBSCAN: the values sorted per key
  unsigned long long *wval;
  long long *wt;
  unsigned long long *wh;   // NULL without DBSCAN
};
inline WinPts win_pts_layout(Carve &c, uint64_t P, bool dbscan) {
  WinPts w;
  w.wval = c.take<unsigned long long>(P);
  w.wt = c.take<long long>(P);
  w.wh = dbscan ? c.take<unsigned long long>(P) : nullptr;
  return w;
}

// ---- tad_run_state_since / tad_drop_state_since (sn_key, sn_pts): the reported suffix of every key of the view ----
struct SinceKeys {   // per key: the suffix's first index | its length | its chunks | the packed offsets | the chunk offsets | a host key_since staged
  uint32_t *first, *cnt, *chunks;
  unsigned long long *poff, *coff;
  long long *since;   // NULL unless staged
};
inline SinceKeys since_keys_layout(Carve &c, uint64_t K, bool staged) {
  SinceKeys k;
  k.first = take_counts(c, K);
  k.cnt = take_counts(c, K);
  k.chunks = take_counts(c, K);
  k.poff = take_offsets(c, K);
  k.coff = take_offsets(c, K);
  k.since = staged ? c.take<long long>(K ? K : 1) : nullptr;
  return k;
}
struct SincePts {   // per reported point: key | value | time
  unsigned long long *nk, *nv;
  long long *nt;
};
inline SincePts since_pts_layout(Carve &c, uint64_t P) {
  SincePts p;
  p.nk = c.take<unsigned long long>(P);
  p.nv = c.take<unsigned long long>(P);
  p.nt = c.take<long long>(P);
  return p;
}

// ---- tad_run_state_buckets (bk_key; the bucketed values, times and sorted values are a WinPts over the buckets in wv_pts) ----
// (this layout's stand-alone check lives in tests/test_state_buckets_abi.py)
struct BucketKeys {   // per key: buckets | points folded away or cut | bucket offsets; per chunk of k_win_bucket_fold: heads | their scan (chunks + 1)
  uint32_t *bcnt, *becnt;
  unsigned long long *boff;
  uint32_t *hcnt;
  unsigned long long *hoff;
};
inline BucketKeys bucket_keys_layout(Carve &c, uint64_t K, uint64_t chunks) {
  BucketKeys b;
  b.bcnt = take_counts(c, K);
  b.becnt = take_counts(c, K);
  b.boff = take_offsets(c, K);
  b.hcnt = take_counts(c, chunks);
  b.hoff = take_offsets(c, chunks);
  return b;
}

// ---- tad_state_rollup (bk_key; the folded values and times go straight into the state's candidate arenas) ----
// (this layout's stand-alone check lives in tests/test_state_rollup_abi.py)
struct RollupCounters {   // one 64-byte block on the device, zeroed per call
  unsigned long long rolled, buckets, keys_changed, pad[5];   // raw points below the bound | points below it afterwards | keys that lost a point
};
struct RollupKeys {   // counters | per key: range begin (0) | range length | points afterwards | points folded away | chunks (later the long-sort list) | the list's length | chunk offsets; per chunk: heads | their scan (chunks + 1)
  RollupCounters *rc;
  uint32_t *beg, *len, *rcnt, *ecnt, *chunks;
  unsigned int *long_count;
  unsigned long long *coff;
  uint32_t *hcnt;
  unsigned long long *hoff;
};
inline RollupKeys rollup_keys_layout(Carve &c, uint64_t K, uint64_t chunks) {
  RollupKeys r;
  r.rc = c.take<RollupCounters>(1, 16);
  r.beg = take_counts(c, K);
  r.len = take_counts(c, K);
  r.rcnt = take_counts(c, K);
  r.ecnt = take_counts(c, K);
  r.chunks = take_counts(c, K);
  r.long_count = take_cell(c);
  r.coff = take_offsets(c, K);
  r.hcnt = take_counts(c, chunks);
  r.hoff = take_offsets(c, chunks);
  return r;
}

// ---- tad_state_merge (mg_pts, mg_keys) ----
struct MergeCounters {   // one 64-byte block on the device, zeroed per attempt
  unsigned long long too_old, appended, inserted, combined, keys_touched, keys_replayed, keys_emptied, pad[1];   // keys_emptied: tad_state_replace only
};
struct MergePts {   // per batch point (pc = the batch's bound, at least 1)
  unsigned long long *nhoff, *aoff, *roff;            // the three scans (pc + 1 entries used, pc + 2 held)
  unsigned long long *hadd, *hadd_s, *hrem, *hrem_s;  // the history's gains, sorted | losses, sorted
  uint32_t *rank, *f_nh, *f_kept, *f_hit;             // rank and the flags of the three scans
  uint8_t *cls;
};
inline MergePts merge_pts_layout(Carve &c, uint64_t pc) {
  MergePts m;
  m.nhoff = c.take<unsigned long long>(pc + 2);
  m.aoff = c.take<unsigned long long>(pc + 2);
  m.roff = c.take<unsigned long long>(pc + 2);
  m.hadd = c.take<unsigned long long>(pc);
  m.hadd_s = c.take<unsigned long long>(pc);
  m.hrem = c.take<unsigned long long>(pc);
  m.hrem_s = c.take<unsigned long long>(pc);
  m.rank = c.take<uint32_t>(pc);
  m.f_nh = c.take<uint32_t>(pc);
  m.f_kept = c.take<uint32_t>(pc);
  m.f_hit = c.take<uint32_t>(pc);
  m.cls = c.take<uint8_t>(pc);
  c.pad(16);   // unexplained, kept
  c.pad(64);   // unexplained, kept
  return m;
}
struct MergeKeys {   // per key: counters | long-list length | five offset arrays | four u32 arrays
  MergeCounters *mcnt;
  unsigned int *long_count;
  unsigned long long *akoff, *rkoff, *hoff_mid, *coff_s, *coff_h;
  uint32_t *chunks_s, *chunks_h, *replay, *long_list;
};
inline MergeKeys merge_keys_layout(Carve &c, uint64_t K) {
  MergeKeys m;
  m.mcnt = c.take<MergeCounters>(1);
  m.long_count = take_cell(c);   // (the offsets start at byte 128)
  m.akoff = take_offsets(c, K);
  m.rkoff = take_offsets(c, K);
  m.hoff_mid = take_offsets(c, K);
  m.coff_s = take_offsets(c, K);
  m.coff_h = take_offsets(c, K);
  m.chunks_s = take_counts(c, K);
  m.chunks_h = take_counts(c, K);
  m.replay = take_counts(c, K);
  m.long_list = take_counts(c, K);
  return m;
}

// ---- tad_state_replace (rp_keys, rp_loss), beside a merge's mg_pts / mg_keys ----
struct ReplaceKeys {   // per key: the erased run [ebeg, eend) of its old segment | the old points it loses without a batch point | their scan | zeros
  uint32_t *ebeg, *eend, *ecnt;
  unsigned long long *eoff;
  unsigned long long *pzero;   // K + 1 zeros: the point offsets of a batch without points
};
inline ReplaceKeys replace_keys_layout(Carve &c, uint64_t K) {
  ReplaceKeys r;
  r.ebeg = take_counts(c, K);
  r.eend = take_counts(c, K);
  r.ecnt = take_counts(c, K);
  r.eoff = take_offsets(c, K);
  r.pzero = take_offsets(c, K);
  return r;
}
struct ReplaceLoss {   // the values the history loses (replaced points' old values and erased points), packed per key | sorted per key
  unsigned long long *hrem, *hrem_s;
};
inline ReplaceLoss replace_loss_layout(Carve &c, uint64_t n) {
  ReplaceLoss l;
  l.hrem = c.take<unsigned long long>(n);
  l.hrem_s = c.take<unsigned long long>(n);
  return l;
}

// ---- the change report of a merge or a replace (mg_report; tad_state_merge_changes / tad_state_replace_changes) ----
struct ChangeCounters {   // one 64-byte block on the device, set per attempt by the report's fill kernel
  unsigned long long points, keys;   // changed points | keys with a changed point
  long long min_t, max_t;            // smallest / largest changed time (INT64_MAX / INT64_MIN: none)
  unsigned long long pad[4];
};
struct MergeReport {   // counters | per key: the smallest changed time (staged == false: the caller's own device array is written)
  ChangeCounters *cc;
  long long *since;
};
inline MergeReport merge_report_layout(Carve &c, uint64_t K, bool staged) {
  MergeReport r;
  r.cc = c.take<ChangeCounters>(1);
  r.since = staged ? c.take<long long>(K ? K : 1) : nullptr;
  return r;
}

// ---- a stream ARIMA batch (as_key, as_pt, as_ser, as_pos, as_fit) ----
struct ArimaSlots {
  uint32_t *key;                 // the slot's key
  unsigned long long *yoff;      // its series in the packed Box-Cox arrays (a multiple of 8)
  double *lam, *sigma;           // lambda; stddev_samp from the post-batch moments
  unsigned long long *ibase;     // new-point index of position 0 (wrapping)
  uint32_t *lo, *hi;             // the positions of its fits [lo, hi) (empty without a result)
  uint8_t *ok;                   // 1: the key has a result
};
struct ArimaKeys {   // per key: touched | len8 | slot of the key | its packed offset | the longest touched series; then per slot
  uint32_t *touched, *len8;
  unsigned long long *tidx, *yoffk;
  unsigned int *tmax;
  ArimaSlots sl;
};
inline ArimaKeys arima_keys_layout(Carve &c, uint64_t K) {
  const size_t kpad = kpad4(K);
  ArimaKeys a;
  a.touched = take_counts(c, K);
  a.len8 = take_counts(c, K);
  a.tidx = take_offsets(c, K);
  a.yoffk = take_offsets(c, K);
  a.tmax = take_cell(c);
  a.sl.yoff = c.take<unsigned long long>(kpad, 16);
  a.sl.lam = c.take<double>(kpad, 16);
  a.sl.sigma = c.take<double>(kpad, 16);
  a.sl.ibase = c.take<unsigned long long>(kpad, 16);
  a.sl.key = take_counts(c, K);
  a.sl.lo = take_counts(c, K);
  a.sl.hi = take_counts(c, K);
  a.sl.ok = c.take<uint8_t>(kpad);
  c.pad(256);   // unexplained, kept
  return a;
}
struct ArimaPts {   // per new point: prediction | rows | row offsets (P + 1) | verdict
  double *pcalc;
  uint32_t *rows;
  unsigned long long *row_off;
  uint8_t *pflag;
};
inline ArimaPts arima_pts_layout(Carve &c, uint64_t P) {
  const size_t ppad = (size_t)((P + 3) & ~3ull);
  ArimaPts a;
  a.pcalc = c.take<double>(ppad, 16);
  a.rows = c.take<uint32_t>(ppad, 16);
  a.row_off = c.take<unsigned long long>(ppad + 4, 16);
  a.pflag = c.take<uint8_t>(ppad);
  c.pad(32);   // the block was sized ppad * 21 + 64: 32 of the 64 are row_off's four extra entries above, these 32 are unexplained, kept
  return a;
}
struct ArimaSeries {   // the packed Box-Cox series: lx | ysk, `ser` doubles each
  double *lx, *ysk;
  size_t ser;          // S8 + tmax and the slack behind them (the stride of the two arrays; ysk is zeroed over all of it)
};
inline ArimaSeries arima_series_layout(Carve &c, uint64_t S8, uint32_t tmax) {
  const size_t len = (size_t)S8 + tmax;
  ArimaSeries a;
  a.ser = len + 32;
  a.lx = c.take<double>(len);
  c.pad(32 * sizeof(double));   // what an idle lane's staged loads may touch (k_arima_fit_list reads slot 0's offset up to the wavefront's position + 16)
  a.ysk = c.take<double>(len);
  c.pad(32 * sizeof(double));   // the same, zeroed with the array: finite values for idle lanes
  return a;
}
struct ArimaPos {   // per position: fits | (64-byte aligned) first fit of each position (npos + 1)
  unsigned int *pcnt;
  unsigned long long *loff;
};
inline ArimaPos arima_pos_layout(Carve &c, uint64_t npos) {
  ArimaPos a;
  a.pcnt = c.take<unsigned int>(npos, 64);
  const size_t gap = c.pad_to(64);   // loff starts on the next 64-byte boundary: 0 .. 60 bytes
  a.loff = c.take<unsigned long long>(npos + 1, 64);
  // The block was sized npos * 12 + 128 whatever the gap.  Of the 128, 8 are loff's entry npos and `gap` went above; the rest (60 .. 120
  // bytes) is unexplained, kept
  c.pad(128 - 8 - gap);
  return a;
}
struct ArimaFits {   // per fit: slot | position; per wavefront: position
  uint32_t *list, *fpos, *wpos;
};
inline ArimaFits arima_fits_layout(Carve &c, uint64_t nfits, uint64_t waves) {
  const size_t fpad = (size_t)((nfits + 3) & ~3ull);
  ArimaFits a;
  a.list = c.take<uint32_t>(fpad, 16);
  a.fpos = c.take<uint32_t>(fpad, 16);
  a.wpos = c.take<uint32_t>(waves + 4, 16);
  c.pad(64);   // unexplained, kept
  return a;
}

// ---- the drop detector on a state (ds_key, ds_pt) ----
struct DropStateKeys {   // per key
  double *mean, *std, *m2;   // pairwise mean, pandas' sample std, the pairwise sum of (mean - x)^2
  uint32_t *n;               // the key's points
  uint8_t *ok;               // 1: the key has a result (n >= min_samples && n >= 2)
};
inline DropStateKeys drop_state_keys_layout(Carve &c, uint64_t K) {
  const size_t kpad = kpad8(K);
  DropStateKeys d;
  d.mean = c.take<double>(kpad);
  d.std = c.take<double>(kpad);
  d.m2 = c.take<double>(kpad);
  d.n = c.take<uint32_t>(kpad);
  d.ok = c.take<uint8_t>(kpad);
  c.pad(64);   // unexplained, kept
  return d;
}
struct DropPts {   // per judged point: row offsets (pc + 1) | rows | verdict
  unsigned long long *row;
  uint32_t *cnt;
  uint8_t *flag;
};
inline DropPts drop_pts_layout(Carve &c, uint64_t pc) {
  DropPts d;
  d.row = c.take<unsigned long long>(pc + 1);
  d.cnt = c.take<uint32_t>(pc);
  d.flag = c.take<uint8_t>(pc);
  c.pad(64);   // unexplained, kept
  return d;
}

// ---- the sparse Stage 0 (sp_temp, sp_cls, the class tables) ----
struct SparseTemp {   // the sort's temporary storage (tb bytes, a 256-byte multiple) | unique points, longest series
  void *temp;
  unsigned long long *runs;
};
inline SparseTemp sparse_temp_layout(Carve &c, size_t tb) {
  SparseTemp t;
  t.temp = c.take<unsigned char>(tb);
  t.runs = c.take<unsigned long long>(2, 16);
  c.pad(48);   // unexplained, kept
  return t;
}
struct StreamPoints {   // a sparse streaming batch: per-key points | their offsets (K + 1)
  uint32_t *len;
  unsigned long long *poff;
};
inline StreamPoints stream_points_layout(Carve &c, uint64_t K) {
  StreamPoints p;
  p.len = take_counts(c, K);
  p.poff = c.take<unsigned long long>(K + 1, 16);
  c.pad(64);   // unexplained, kept
  return p;
}
struct ClassKeys {   // the length classes, per key: points | member of the class | its points | class key offsets | class point offsets
  uint32_t *len, *member, *pts;
  unsigned long long *key_off, *pt_off;
};
inline ClassKeys class_keys_layout(Carve &c, uint64_t K) {
  ClassKeys k;
  k.len = take_counts(c, K);
  k.member = take_counts(c, K);
  k.pts = take_counts(c, K);
  k.key_off = take_offsets(c, K);
  k.pt_off = take_offsets(c, K);
  c.pad(64);   // unexplained, kept
  return k;
}
struct ClassTables {   // three 8-byte columns per point, class after class, then the key maps (class key -> original key)
  unsigned long long *key;
  long long *t;
  unsigned long long *val;
  uint32_t *map;
};
inline ClassTables class_tables_layout(Carve &c, uint64_t P, uint64_t kmax) {
  ClassTables t;
  t.key = c.take<unsigned long long>(P);
  t.t = c.take<long long>(P);
  t.val = c.take<unsigned long long>(P);
  t.map = c.take<uint32_t>(kmax);
  c.pad(256);   // unexplained, kept
  return t;
}

// ---- tad_drop_select's workspace (dsel): every part rounded up to 256 bytes ----
struct DselDims {
  uint64_t n, words, tiles, scan_elems;   // rows | 16-row words of the bitmask | tiles | the tile scan's scratch
  bool t32;                               // 4-byte times
  bool host, has_end, has_keep;           // a host table is staged behind the rest: its flow_end_s / keep columns are optional
};
struct DselWs {
  uint16_t *bits;
  uint32_t *cnt;
  unsigned long long *off, *scratch, *total;
  // a host table's columns (NULL for a device table)
  uint8_t *ia, *ea;
  void *ts, *te;
  long long *codes[6];
  uint8_t *keep;
};
inline DselWs dsel_layout(Carve &c, const DselDims &d) {
  DselWs w{};
  const size_t n = (size_t)d.n, tbytes = n * (d.t32 ? 4 : 8);
  w.bits = c.take<uint16_t>(d.words, 256); c.pad_to(256);
  w.cnt = c.take<uint32_t>(d.tiles, 256); c.pad_to(256);
  w.off = c.take<unsigned long long>(d.tiles + 1, 256); c.pad_to(256);
  w.scratch = c.take<unsigned long long>(d.scan_elems, 256); c.pad_to(256);
  w.total = c.take<unsigned long long>(1, 256); c.pad_to(256);
  if (!d.host) return w;
  w.ia = c.take<uint8_t>(n, 256); c.pad_to(256);
  w.ea = c.take<uint8_t>(n, 256); c.pad_to(256);
  w.ts = c.take<unsigned char>(tbytes, 256); c.pad_to(256);
  if (d.has_end) { w.te = c.take<unsigned char>(tbytes, 256); c.pad_to(256); }
  for (int i = 0; i < 6; ++i) { w.codes[i] = c.take<long long>(n, 256); c.pad_to(256); }
  if (d.has_keep) { w.keep = c.take<uint8_t>(n, 256); c.pad_to(256); }
  return w;
}

// ---- the dictionaries' decode side (tad_keydict_gather, tad_strdict_decode): every part rounded up to 256 bytes ----
struct KdGatherWs {   // the flag word; a host call's staging behind it: the ids | the asked columns | the sides
  uint32_t *flags;
  unsigned long long *ids;   // NULL for a device call, as are the columns and the sides
  long long *col[8];         // (kFzMaxCols) NULL where the caller's entry is
  uint8_t *side;
};
inline KdGatherWs kd_gather_layout(Carve &c, uint64_t n, int n_cols, unsigned col_mask, bool with_side, bool host) {
  KdGatherWs w{};
  w.flags = c.take<uint32_t>(1, 256); c.pad_to(256);
  if (!host) return w;
  w.ids = c.take<unsigned long long>((size_t)n, 256); c.pad_to(256);
  for (int i = 0; i < n_cols && i < 8; ++i)
    if (col_mask & (1u << i)) { w.col[i] = c.take<long long>((size_t)n, 256); c.pad_to(256); }
  if (with_side) { w.side = c.take<uint8_t>((size_t)n, 256); c.pad_to(256); }
  return w;
}
struct SdDecodeWs {   // the flag word | a host call's codes | lengths | offsets (n + 1: the scan's total is the last)
  uint32_t *flags;
  long long *codes;   // NULL when the codes are device memory
  uint32_t *cnt;
  unsigned long long *off;
};
inline SdDecodeWs sd_decode_layout(Carve &c, uint64_t n, bool host_codes) {
  SdDecodeWs w{};
  w.flags = c.take<uint32_t>(1, 256); c.pad_to(256);
  if (host_codes) { w.codes = c.take<long long>((size_t)n, 256); c.pad_to(256); }
  w.cnt = c.take<uint32_t>((size_t)n, 256); c.pad_to(256);
  w.off = c.take<unsigned long long>((size_t)n + 1, 256); c.pad_to(256);
  return w;
}
// tad_strdict_compact over K values: the survivor count's cell | a host call's keep | a host call's remap | live | units | new codes
// (K + 1) | new arena offsets in 16-byte units (K + 1) | the survivors' old offsets in 16-byte units, by new code
struct SdCompactWs {
  uint32_t *flags;
  uint8_t *keep;      // NULL when keep is device memory
  long long *remap;   // NULL when remap is device memory
  uint32_t *live, *units;
  unsigned long long *newcode, *off16, *src16;
};
inline SdCompactWs sd_compact_layout(Carve &c, uint64_t K, bool host_keep, bool host_remap) {
  SdCompactWs w{};
  w.flags = c.take<uint32_t>(1, 256); c.pad_to(256);
  if (host_keep) { w.keep = c.take<uint8_t>((size_t)K, 256); c.pad_to(256); }
  if (host_remap) { w.remap = c.take<long long>((size_t)K, 256); c.pad_to(256); }
  w.live = c.take<uint32_t>((size_t)K, 256); c.pad_to(256);
  w.units = c.take<uint32_t>((size_t)K, 256); c.pad_to(256);
  w.newcode = c.take<unsigned long long>((size_t)K + 1, 256); c.pad_to(256);
  w.off16 = c.take<unsigned long long>((size_t)K + 1, 256); c.pad_to(256);
  w.src16 = c.take<unsigned long long>((size_t)K, 256); c.pad_to(256);
  return w;
}
// tad_keydict_mark_codes: the count | the flag word; a host call's used bytes behind them
struct KdMarkWs {
  unsigned long long *n_used;
  uint32_t *flags;
  uint8_t *used;      // NULL when used is device memory
};
inline KdMarkWs kd_mark_layout(Carve &c, uint64_t used_len, bool host) {
  KdMarkWs w{};
  w.n_used = c.take<unsigned long long>(1, 256);
  w.flags = c.take<uint32_t>(1); c.pad_to(256);
  if (host) { w.used = c.take<uint8_t>((size_t)used_len, 256); c.pad_to(256); }
  return w;
}
// tad_keydict_recode: the flag word; a host call's remaps behind it, term by term
struct KdRecodeWs {
  uint32_t *flags;
  long long *remap[8];   // NULL: the term's remap is device memory (or the term does not exist)
};
inline KdRecodeWs kd_recode_layout(Carve &c, int n_terms, const uint64_t *remap_len, bool host) {
  KdRecodeWs w{};
  w.flags = c.take<uint32_t>(1, 256); c.pad_to(256);
  if (host)
    for (int t = 0; t < n_terms && t < 8; ++t) { w.remap[t] = c.take<long long>((size_t)remap_len[t], 256); c.pad_to(256); }
  return w;
}

}  // namespace tad

#endif  // THEIA_TAD_CARVE_H
