// tad_capi_state.cpp — the life of a streaming state (include/tad.h: tad_state_*): create, destroy, export / import of the moments, the
// history, the series and the times, resize, trim, compact, and what the batches on a state (tad_capi.cpp) share with them.  Everything a
// state holds is double-buffered and indexed by tad_state::cur (tad_engine.h); every step that applies to "each store the state keeps"
// is written once here, over each_segments / each_arena.
#include "tad_bucket.h"
#include "tad_engine.h"

using namespace tad;
using namespace tadh;

namespace {

// The segment sets the state keeps — history, series — as members of tad_state: f(m), so that a caller with two states (the old and the
// grown one of a resize) reaches the same set in both.
template <typename S, typename F> void each_segments(S *st, F f) {
  if (st->history) f(&tad_state::hist);
  if (st->series) f(&tad_state::ser);
}

// Every value arena the state keeps — series, times, history — with the segments whose offsets and lengths it follows and its name in
// messages: f(arena, segments, what), until one fails.
template <typename S, typename F> int each_arena(S *st, F f) {
  int rc = TAD_OK;
  if (st->series) rc = f(st->ser.val, st->ser, "series");
  if (rc == TAD_OK && st->times) rc = f(st->ser_times, st->ser, "times");
  if (rc == TAD_OK && st->history) rc = f(st->hist.val, st->hist, "history");
  return rc;
}

// copy `i` of an arena — a candidate: the current copy is never touched, so a failure leaves the state as it is — given back and, with
// want != 0, allocated anew for `want` values; false: out of memory (*r says why)
template <typename T> bool renew_arena(Arena<T> &a, int i, uint64_t want, hipError_t *r) {
  if (a.p[i]) hipFree(a.p[i]);
  a.p[i] = nullptr;
  a.cap[i] = 0;
  void *p = nullptr;
  if (want == 0) return true;
  if ((*r = hipMalloc(&p, want * sizeof(T))) != hipSuccess) { (void)hipGetLastError(); return false; }
  a.p[i] = static_cast<T *>(p);
  a.cap[i] = want;
  return true;
}

// copy `i` of an arena grows to hold `need` values, geometrically
template <typename T> int grow_arena(JobCtx *e, Arena<T> &a, int i, uint64_t need, const char *what) {
  if (a.cap[i] >= need) return TAD_OK;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  hipError_t r;
  if (!renew_arena(a, i, need > 2 * a.cap[i] ? need : 2 * a.cap[i], &r))
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_run_stream: %llu values of %s do not fit (%s); state unchanged", (unsigned long long)need, what,
                hipGetErrorString(r));
  return TAD_OK;
}

// a trim leaves `len` values in copy `i` of an arena: below a quarter of its capacity the copy is given back and, for a candidate that is
// about to be written, allocated anew at twice the length (how a trimmed state's memory actually shrinks); a candidate too small grows to
// twice the length too.
template <typename T> int size_trim_arena(JobCtx *e, Arena<T> &a, int i, uint64_t len, bool allocate, const char *who) {
  if (a.cap[i] >= len && !(len * 4 < a.cap[i])) return TAD_OK;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  hipError_t r;
  if (!renew_arena(a, i, allocate ? 2 * len : 0, &r))
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "%s: %llu retained values do not fit (%s); state unchanged", who, (unsigned long long)len, hipGetErrorString(r));
  return TAD_OK;
}

// Copy `i` of every arena sized for what a trim or compact leaves: the candidates before they are written (allocate), the old current
// ones — candidates by then — after the commit.
int size_arenas(JobCtx *e, tad_state *st, int i, uint64_t n_ser, uint64_t n_hist, bool allocate, const char *who) {
  return each_arena(st, [&](auto &a, const Segments &seg, const char *) {
    return size_trim_arena(e, a, i, &seg == &st->hist ? n_hist : n_ser, allocate, who);
  });
}

// What a state holds per key, for K keys and all zero (every key unseen, every segment empty): both moment blocks (blocks) and both copies
// of every offset array it keeps.  A failure leaves what was allocated to free_keyed.
hipError_t alloc_keyed(tad_state *st, uint64_t K, hipStream_t s, bool blocks = true) {
  hipError_t r = hipSuccess;
  auto zeroed = [&](void **p, size_t bytes) {
    if (r == hipSuccess) r = hipMalloc(p, bytes);
    if (r == hipSuccess) r = hipMemsetAsync(*p, 0, bytes, s);
  };
  for (int i = 0; i < 2; ++i) {
    if (blocks) zeroed(&st->block[i], state_bytes(K));   // n = 0, avg = m2 = ewma = 0, unseen
    each_segments(st, [&](auto m) { zeroed(reinterpret_cast<void **>(&(st->*m).off[i]), (K + 1) * 8); });
  }
  return r;
}

void free_keyed(tad_state *st) {
  for (int i = 0; i < 2; ++i) {
    if (st->block[i]) hipFree(st->block[i]);
    each_segments(st, [&](auto m) { if ((st->*m).off[i]) hipFree((st->*m).off[i]); });
  }
}

// the blocks and offsets of `from` (its K keys, the same flags) replace the state's own, which are freed: the last step of a resize or compact
void adopt_keyed(tad_state *st, const tad_state *from) {
  free_keyed(st);
  for (int i = 0; i < 2; ++i) {
    st->block[i] = from->block[i];
    each_segments(st, [&](auto m) { (st->*m).off[i] = (from->*m).off[i]; });
  }
  st->K = from->K;
}

// the current copy of everything moves to index 0
void current_to_front(tad_state *st) {
  if (st->cur == 0) return;
  std::swap(st->block[0], st->block[1]);
  each_segments(st, [&](auto m) { std::swap((st->*m).off[0], (st->*m).off[1]); std::swap((st->*m).len[0], (st->*m).len[1]); });
  each_arena(st, [](auto &a, const Segments &, const char *) { a.swap(); return TAD_OK; });
  st->cur = 0;
}

// `total` values from the host into copy `cand` of an arena, grown to fit when too small; the caller swaps the copies once everything
// that goes with them has arrived
template <typename T> int fill_candidate(JobCtx *e, Arena<T> &a, int cand, const void *src, uint64_t total, const char *who) {
  if (a.cap[cand] < total) {
    void *p = nullptr;
    const hipError_t r = hipMalloc(&p, total * 8);
    if (r != hipSuccess) { (void)hipGetLastError(); return fail(e, TAD_ERR_OUT_OF_MEMORY, "%s: %s; state unchanged", who, hipGetErrorString(r)); }
    if (a.p[cand]) hipFree(a.p[cand]);
    a.p[cand] = static_cast<T *>(p);
    a.cap[cand] = total;
  }
  if (total) HIP_TRY(e, hipMemcpy(a.p[cand], src, total * 8, hipMemcpyHostToDevice));
  return TAD_OK;
}

// The history and the series behind tad_state_{history,series}_points, _export_* and _import_*: the two differ in these names, in that
// a history's values ascend and in that a new series waits for its times.
struct Kind {
  Segments tad_state::*seg;
  bool tad_state::*kept;
  const char *noun, *flag;
};
constexpr Kind kHistory{&tad_state::hist, &tad_state::history, "history", "TAD_STATE_HISTORY"};
constexpr Kind kSeries{&tad_state::ser, &tad_state::series, "series", "TAD_STATE_SERIES"};

int segments_points(tad_engine *eng, const tad_state *st, const Kind &kd, uint64_t *n_points) {
  if (!eng || !st || !n_points) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_%s_points: bad arguments", kd.noun);
  std::lock_guard<std::mutex> state_lk(st->mu);
  *n_points = st->*kd.kept ? (st->*kd.seg).len[st->cur] : 0;
  return TAD_OK;
}

// what an export or import refuses before it takes the state's lock (who: the call's name)
int segments_check(tad_engine *eng, const tad_state *st, const Kind &kd, const char *who, const uint64_t *len) {
  if (!eng || !st || !len) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (!(st->*kd.kept)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state has no %s (%s)", who, kd.noun, kd.flag);
  return TAD_OK;
}

// every key's length from the current offsets, then the values
int export_segments(tad_engine *eng, const tad_state *st, const Kind &kd, const char *who, uint64_t *len, uint64_t *values) {
  int rc = segments_check(eng, st, kd, who, len);
  if (rc != TAD_OK) return rc;
  StateCall call(eng, st);
  if ((rc = call.enter(who)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  const Segments &seg = st->*kd.seg;
  std::vector<unsigned long long> off;
  try { off.resize(st->K + 1); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  HIP_TRY(e, hipMemcpy(off.data(), seg.off[st->cur], (st->K + 1) * 8, hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < st->K; ++k) len[k] = off[k + 1] - off[k];
  const uint64_t total = seg.len[st->cur];
  if (values && total) HIP_TRY(e, hipMemcpy(values, seg.val.p[st->cur], total * 8, hipMemcpyDeviceToHost));
  return TAD_OK;
}

// len[k] values for key k, which must be the n[k] of its moments.  Into the candidate copy, which then trades places with the current
// one: any failure leaves the segments as they were.
int import_segments(tad_engine *eng, tad_state *st, const Kind &kd, const char *who, const uint64_t *len, const uint64_t *values) {
  int rc = segments_check(eng, st, kd, who, len);
  if (rc != TAD_OK) return rc;
  StateCall call(eng, st);
  if ((rc = call.enter(who)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  Segments &seg = st->*kd.seg;
  const uint64_t K = st->K;
  std::vector<uint32_t> n;
  std::vector<unsigned long long> off;
  try { n.resize(K); off.resize(K + 1); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  HIP_TRY(e, hipMemcpy(n.data(), state_view(st, st->cur).n, K * sizeof(uint32_t), hipMemcpyDeviceToHost));
  off[0] = 0;
  for (uint64_t k = 0; k < K; ++k) {
    if (len[k] != n[k])
      return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: key %llu has %llu values, its state has n = %u (import the moments first); state unchanged", who,
                  (unsigned long long)k, (unsigned long long)len[k], n[k]);
    off[k + 1] = off[k] + len[k];
  }
  const uint64_t total = off[K];
  if (total && !values) return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: values is NULL", who);
  if (&kd == &kHistory)
    for (uint64_t k = 0; k < K; ++k)
      for (uint64_t i = off[k] + 1; i < off[k + 1]; ++i)
        if (values[i] < values[i - 1])
          return fail(e, TAD_ERR_INVALID_ARGUMENT, "%s: the values of key %llu are not ascending; state unchanged", who, (unsigned long long)k);
  const int cand = st->cur ^ 1;
  if ((rc = fill_candidate(e, seg.val, cand, values, total, who)) != TAD_OK) return rc;
  HIP_TRY(e, hipMemcpy(seg.off[cand], off.data(), (K + 1) * 8, hipMemcpyHostToDevice));
  std::swap(seg.off[0], seg.off[1]);
  seg.val.swap();
  seg.len[st->cur] = total;
  if (&kd == &kSeries) st->times_stale = st->times;   // the times of a times state come next (tad_state_import_times)
  return TAD_OK;
}

}  // namespace

namespace tadh {

StreamState state_view(const tad_state *st, int which) { return stream_view(st->block[which], st->K); }

// copy `which` of a series state as the detectors of tad_run_state read it (the times and the history where the state has them)
StateView series_view(const tad_state *st, int which) {
  StateView v;
  v.K = st->K;
  v.P = st->ser.len[which];
  v.soff = st->ser.off[which];
  v.sval = st->ser.val.p[which];
  v.st = st->times ? st->ser_times.p[which] : nullptr;
  v.mom = state_view(st, which);
  if (st->history) { v.hoff = st->hist.off[which]; v.hval = st->hist.val.p[which]; }
  return v;
}

// the candidate arenas hold what the current ones hold plus a batch of at most P_cap points
int state_grow_candidates(JobCtx *e, tad_state *st, uint64_t P_cap) {
  const int cur = st->cur;
  return each_arena(st, [&](auto &a, const Segments &seg, const char *what) { return grow_arena(e, a, cur ^ 1, seg.len[cur] + P_cap, what); });
}

int state_size_arenas(JobCtx *e, tad_state *st, int i, uint64_t n_ser, uint64_t n_hist, bool allocate, const char *who) {
  return size_arenas(e, st, i, n_ser, n_hist, allocate, who);
}

// everything succeeded: the candidate copies, which now hold n_ser series points and n_hist history values, become current
void state_commit(tad_state *st, uint64_t n_ser, uint64_t n_hist) {
  const int cand = st->cur ^ 1;
  if (st->series) st->ser.len[cand] = n_ser;
  if (st->history) st->hist.len[cand] = n_hist;
  st->cur = cand;
}

uint64_t state_device_bytes(const tad_state *st) {
  uint64_t b = 2 * (uint64_t)state_bytes(st->K);
  each_segments(st, [&](auto) { b += 2 * (st->K + 1) * 8; });   // both copies of a key-offset array
  each_arena(st, [&](const auto &a, const Segments &, const char *) { b += (a.cap[0] + a.cap[1]) * 8; return TAD_OK; });
  return b;
}

}  // namespace tadh

extern "C" {

int tad_state_create(tad_engine *eng, uint64_t num_keys, tad_state **out) {
  if (!eng || !out || num_keys == 0) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_create: bad arguments");
  *out = nullptr;
  Lease lease(eng);
  JobCtx *e = lease.c;
  if (!e) return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_state_create: no job context available");
  HIP_TRY(e, hipSetDevice(e->device));
  tad_state *st = new (std::nothrow) tad_state();
  if (!st) return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory");
  st->K = num_keys;
  const hipError_t r = alloc_keyed(st, num_keys, e->stream);
  if (r != hipSuccess) {
    free_keyed(st);
    delete st;
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_state_create: %s", hipGetErrorString(r));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  *out = st;
  return TAD_OK;
}

void tad_state_destroy(tad_engine *e, tad_state *st) {
  if (!st) return;
  { std::lock_guard<std::mutex> lk(st->mu); }   // a batch on this state has returned (it synchronises its stream before it does)
  if (e) hipSetDevice(e->device);
  free_keyed(st);
  each_arena(st, [](auto &a, const Segments &, const char *) {
    for (int i = 0; i < 2; ++i)
      if (a.p[i]) hipFree(a.p[i]);
    return TAD_OK;
  });
  delete st;
}

int tad_state_export(tad_engine *eng, const tad_state *st, uint32_t *n, double *avg, double *m2, double *ewma, int64_t *last_t) {
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_export: bad arguments");
  StateCall call(eng, st);
  int rc;
  if ((rc = call.enter("tad_state_export")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  const StreamState v = state_view(st, st->cur);
  if (n) HIP_TRY(e, hipMemcpy(n, v.n, st->K * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (avg) HIP_TRY(e, hipMemcpy(avg, v.avg, st->K * sizeof(double), hipMemcpyDeviceToHost));
  if (m2) HIP_TRY(e, hipMemcpy(m2, v.m2, st->K * sizeof(double), hipMemcpyDeviceToHost));
  if (ewma) HIP_TRY(e, hipMemcpy(ewma, v.ewma, st->K * sizeof(double), hipMemcpyDeviceToHost));
  if (last_t) HIP_TRY(e, hipMemcpy(last_t, v.last_t, st->K * sizeof(long long), hipMemcpyDeviceToHost));
  return TAD_OK;
}

int tad_state_resize(tad_engine *eng, tad_state *st, uint64_t new_num_keys) {
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_resize: bad arguments");
  StateCall call(eng, st);
  if (new_num_keys < st->K)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_resize: %llu keys < the %llu the state holds (a state only grows)",
                (unsigned long long)new_num_keys, (unsigned long long)st->K);
  if (new_num_keys == st->K) return TAD_OK;
  int rc;
  if ((rc = call.enter("tad_state_resize")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  // blocks and offsets anew (the old ones stay the state's until everything succeeded); the added keys are unseen (all zeros)
  tad_state grown;
  grown.K = new_num_keys;
  grown.history = st->history;
  grown.series = st->series;
  const size_t K = st->K;
  const int cur = st->cur;
  hipError_t r = alloc_keyed(&grown, new_num_keys, e->stream);
  auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (r == hipSuccess) r = hipMemcpyAsync(dst, src, bytes, kind, e->stream);
  };
  if (r == hipSuccess) {
    const StreamState a = state_view(st, cur), b = state_view(&grown, 0);
    copy(b.avg, a.avg, K * sizeof(double), hipMemcpyDeviceToDevice);
    copy(b.m2, a.m2, K * sizeof(double), hipMemcpyDeviceToDevice);
    copy(b.ewma, a.ewma, K * sizeof(double), hipMemcpyDeviceToDevice);
    copy(b.last_t, a.last_t, K * sizeof(long long), hipMemcpyDeviceToDevice);
    copy(b.n, a.n, K * sizeof(uint32_t), hipMemcpyDeviceToDevice);
    copy(b.seen, a.seen, K, hipMemcpyDeviceToDevice);
  }
  // copy 0 of the new offsets keeps the current one's and gives the added keys empty segments at the end (offset = the segments' length).
  // The value arenas stay; the current ones move to index 0 with the state.
  std::vector<unsigned long long> tail_off[2];   // (the history's, the series': alive until the stream is synchronised)
  int t = 0;
  each_segments(st, [&](auto m) {
    std::vector<unsigned long long> &tail = tail_off[t++];
    try { tail.assign(new_num_keys - K, (st->*m).len[cur]); } catch (...) { if (r == hipSuccess) r = hipErrorOutOfMemory; }
    copy((grown.*m).off[0], (st->*m).off[cur], (K + 1) * 8, hipMemcpyDeviceToDevice);
    copy((grown.*m).off[0] + K + 1, tail.data(), tail.size() * 8, hipMemcpyHostToDevice);
  });
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  if (r != hipSuccess) {
    free_keyed(&grown);
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_state_resize: %s (state unchanged)", hipGetErrorString(r));
  }
  current_to_front(st);
  adopt_keyed(st, &grown);
  return TAD_OK;
}

int tad_state_import(tad_engine *eng, tad_state *st, const uint32_t *n, const double *avg, const double *m2, const double *ewma, const int64_t *last_t) {
  if (!eng || !st || !n || !avg || !m2 || !ewma || !last_t) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_import: bad arguments");
  StateCall call(eng, st);
  int rc;
  if ((rc = call.enter("tad_state_import")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  // the state's layout on the host (state_view), then one copy: a key with n == 0 is unseen and all zeros
  const size_t K = st->K;
  std::vector<unsigned char> h;
  try { h.assign(state_bytes(K), 0); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  const StreamState hv = stream_view(h.data(), K);
  for (size_t k = 0; k < K; ++k) {
    if (n[k] == 0) continue;
    hv.avg[k] = avg[k]; hv.m2[k] = m2[k]; hv.ewma[k] = ewma[k]; hv.last_t[k] = last_t[k]; hv.n[k] = n[k]; hv.seen[k] = 1;
  }
  HIP_TRY(e, hipMemcpy(st->block[st->cur], h.data(), h.size(), hipMemcpyHostToDevice));
  return TAD_OK;
}

int tad_state_create_ex(tad_engine *eng, uint64_t num_keys, uint32_t flags, tad_state **out) {
  const uint32_t known = TAD_STATE_HISTORY | TAD_STATE_SERIES | TAD_STATE_TIMES;
  if (out) *out = nullptr;
  if (flags & ~known) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_create_ex: unknown flags 0x%x", flags & ~known);
  if ((flags & TAD_STATE_TIMES) && !(flags & TAD_STATE_SERIES))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_create_ex: TAD_STATE_TIMES needs TAD_STATE_SERIES");
  int rc = tad_state_create(eng, num_keys, out);
  if (rc != TAD_OK || !(flags & known)) return rc;
  tad_state *st = *out;
  st->history = (flags & TAD_STATE_HISTORY) != 0;
  st->series = (flags & TAD_STATE_SERIES) != 0;
  st->times = (flags & TAD_STATE_TIMES) != 0;   // (the times arenas come with the first batch, like the values)
  // every key's segment empty: offsets all zero (the value arenas come with the first batch); no context is held here: the null stream
  hipError_t r = hipSetDevice(eng->device);
  if (r == hipSuccess) r = alloc_keyed(st, num_keys, nullptr, false);
  if (r == hipSuccess) r = hipStreamSynchronize(nullptr);
  if (r != hipSuccess) {
    tad_state_destroy(eng, st);
    *out = nullptr;
    return fail(eng, TAD_ERR_OUT_OF_MEMORY, "tad_state_create_ex: %s", hipGetErrorString(r));
  }
  return TAD_OK;
}

int tad_state_history_points(tad_engine *eng, const tad_state *st, uint64_t *n_points) { return segments_points(eng, st, kHistory, n_points); }
int tad_state_series_points(tad_engine *eng, const tad_state *st, uint64_t *n_points) { return segments_points(eng, st, kSeries, n_points); }

int tad_state_export_history(tad_engine *eng, const tad_state *st, uint64_t *len, uint64_t *values) {
  return export_segments(eng, st, kHistory, "tad_state_export_history", len, values);
}
int tad_state_export_series(tad_engine *eng, const tad_state *st, uint64_t *len, uint64_t *values) {
  return export_segments(eng, st, kSeries, "tad_state_export_series", len, values);
}

int tad_state_import_history(tad_engine *eng, tad_state *st, const uint64_t *len, const uint64_t *values) {
  return import_segments(eng, st, kHistory, "tad_state_import_history", len, values);
}
int tad_state_import_series(tad_engine *eng, tad_state *st, const uint64_t *len, const uint64_t *values) {
  return import_segments(eng, st, kSeries, "tad_state_import_series", len, values);
}

int tad_state_export_times(tad_engine *eng, const tad_state *st, int64_t *t) {
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_export_times: bad arguments");
  if (!st->times) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_export_times: the state has no times (TAD_STATE_TIMES)");
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_export_times: the series was imported without its times (tad_state_import_times)");
  const uint64_t total = st->ser.len[st->cur];
  if (!total) return TAD_OK;
  if (!t) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_export_times: t is NULL");
  int rc;
  if ((rc = call.enter("tad_state_export_times")) != TAD_OK) return rc;
  HIP_TRY(call.e, hipMemcpy(t, st->ser_times.p[st->cur], total * 8, hipMemcpyDeviceToHost));
  return TAD_OK;
}

int tad_state_import_times(tad_engine *eng, tad_state *st, const int64_t *t) {
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_import_times: bad arguments");
  if (!st->times) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_import_times: the state has no times (TAD_STATE_TIMES)");
  StateCall call(eng, st);
  int rc;
  if ((rc = call.enter("tad_state_import_times")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  const uint64_t K = st->K, total = st->ser.len[st->cur];
  if (total && !t) return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_state_import_times: t is NULL");
  std::vector<long long> last;
  std::vector<unsigned long long> off;
  try { last.resize(K); off.resize(K + 1); } catch (...) { return fail(e, TAD_ERR_OUT_OF_MEMORY, "out of host memory"); }
  HIP_TRY(e, hipMemcpy(off.data(), st->ser.off[st->cur], (K + 1) * 8, hipMemcpyDeviceToHost));
  HIP_TRY(e, hipMemcpy(last.data(), state_view(st, st->cur).last_t, K * sizeof(long long), hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < K; ++k) {
    if (off[k + 1] == off[k]) continue;
    for (uint64_t i = off[k] + 1; i < off[k + 1]; ++i)
      if (t[i] <= t[i - 1])
        return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_state_import_times: the times of key %llu are not strictly ascending; state unchanged",
                    (unsigned long long)k);
    if (t[off[k + 1] - 1] != last[k])
      return fail(e, TAD_ERR_INVALID_ARGUMENT, "tad_state_import_times: the last time of key %llu is %lld, its state has last_t = %lld; state unchanged",
                  (unsigned long long)k, (long long)t[off[k + 1] - 1], last[k]);
  }
  // into the candidate copy, which then trades places with the current one: any failure leaves the times as they were
  if ((rc = fill_candidate(e, st->ser_times, st->cur ^ 1, t, total, "tad_state_import_times")) != TAD_OK) return rc;
  st->ser_times.swap();
  st->times_stale = false;
  return TAD_OK;
}

int tad_state_bytes(tad_engine *eng, const tad_state *st, uint64_t *bytes) {
  if (!eng || !st || !bytes) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_bytes: bad arguments");
  std::lock_guard<std::mutex> state_lk(st->mu);
  *bytes = state_device_bytes(st);
  return TAD_OK;
}

// tad.h: every key keeps a suffix of its series (kernels in tad_history.hip).  Writes only the candidate copies of the moments, offsets
// and arenas; they become current together once every launch has succeeded.
int tad_state_trim(tad_engine *eng, tad_state *st, uint64_t keep_points, int64_t keep_from_t, double ewma_alpha, uint64_t *dropped) {
  if (dropped) *dropped = 0;
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_trim: bad arguments");
  if (!st->series)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_trim: the state has no series (TAD_STATE_SERIES): a history alone does not know "
                                               "which values are oldest; state unchanged");
  if (keep_from_t != 0 && !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_trim: keep_from_t needs a state with times (TAD_STATE_TIMES); state unchanged");
  if (!(ewma_alpha >= 0.0 && ewma_alpha <= 1.0)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_trim: ewma_alpha out of range");
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_trim: the series was imported without its times (tad_state_import_times)");
  const uint64_t K = st->K;
  const int cur = st->cur, cand = cur ^ 1;
  const uint64_t S = st->ser.len[cur];
  if ((keep_points == 0 && keep_from_t == 0) || S == 0) return TAD_OK;
  int rc;
  if ((rc = call.enter("tad_state_trim")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  hipStream_t s = e->stream;
  const double alpha = ewma_alpha == 0.0 ? 0.5 : ewma_alpha;
  TrimKeys tk;
  if ((rc = carve_bufs(e, e->hs_kcnt, e->hs_koff, &tk, trim_keys_layout, K)) != TAD_OK) return rc;
  if ((rc = ensure(e, e->scan_scratch, scan_scratch_elems(K) * sizeof(unsigned long long))) != TAD_OK) return rc;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const Segments &ser = st->ser, &hist = st->hist;
  const long long *t_cur = st->times ? st->ser_times.p[cur] : nullptr;
  // 1. what every key keeps; the candidate series offsets, the packed evicted offsets and the chunk offsets
  launch_trim_keep(s, K, ser.off[cur], keep_from_t != 0 ? t_cur : nullptr, keep_points, (long long)keep_from_t, tk.rcnt, tk.ecnt, tk.chunks);
  launch_scan(s, tk.rcnt, ser.off[cand], K, scratch);
  launch_scan(s, tk.ecnt, tk.eoff, K, scratch);
  launch_scan(s, tk.chunks, tk.coff, K, scratch);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemcpyAsync(e->tail_host, ser.off[cand] + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(e->tail_host + 8, tk.eoff + K, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  unsigned long long kept = 0, evicted = 0;
  memcpy(&kept, e->tail_host, 8);
  memcpy(&evicted, e->tail_host + 8, 8);
  if (evicted == 0) return TAD_OK;   // nothing to drop: the state stays as it is (the candidate offsets are scratch)
  // 2. the candidate arenas at their new size, the evicted values' scratch: an allocation failure leaves the state as it is
  if ((rc = size_arenas(e, st, cand, kept, kept, true, "tad_state_trim")) != TAD_OK) return rc;
  unsigned long long *ev = nullptr, *es = nullptr;
  if (st->history) {
    if ((rc = ensure(e, e->hs_val, evicted * 8)) != TAD_OK) return rc;
    if ((rc = ensure(e, e->hs_sorted, evicted * 8)) != TAD_OK) return rc;
    ev = static_cast<unsigned long long *>(e->hs_val.p);
    es = static_cast<unsigned long long *>(e->hs_sorted.p);
  }
  // 3. the retained suffixes (and the evicted prefixes); 4. the history without the evicted values; 5. the moments
  const uint64_t bound = trim_chunks_bound(K, S);
  launch_trim_copy(s, bound, tk.coff, K, ser.off[cur], ser.val.p[cur], t_cur, ser.off[cand], ser.val.p[cand], st->times ? st->ser_times.p[cand] : nullptr,
                   tk.eoff, ev);
  if (st->history) {
    HIP_TRY(e, hipMemcpyAsync(hist.off[cand], ser.off[cand], (K + 1) * 8, hipMemcpyDeviceToDevice, s));
    launch_hist_sort(s, ev, tk.eoff, K, es, tk.chunks, tk.long_count);
    launch_hist_subtract(s, bound, tk.coff, K, hist.off[cur], hist.val.p[cur], tk.eoff, es, hist.off[cand], hist.val.p[cand], true);
  }
  launch_trim_moments(s, K, tk.rcnt, tk.ecnt, ser.off[cand], ser.val.p[cand], alpha, state_view(st, cur), state_view(st, cand));
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(s));
  // everything succeeded: the candidate becomes current; the old arenas, now the candidates, are given back when far too big for it
  state_commit(st, kept, kept);
  (void)size_arenas(e, st, cur, kept, kept, false, "tad_state_trim");
  if (dropped) *dropped = evicted;
  return TAD_OK;
}

// tad.h: every key's points below the bound fold into their time buckets, the rest stay (kernels in tad_window.hip: the bucket pair of
// tad_run_state_buckets with rollup_start, over every key's whole segment).  A trim's shape: only the candidate copies of the moments,
// offsets and arenas are written — the fold goes straight into the candidate arenas, no packed copy of the state in between — and they
// become current together once every launch has succeeded.
int tad_state_rollup(tad_engine *eng, tad_state *st, int64_t before_t, int64_t bucket_s, int64_t bucket_origin, tad_value_op bucket_op, double ewma_alpha,
                     tad_rollup_stats *stats) {
  const char *who = "tad_state_rollup";
  if (stats) *stats = tad_rollup_stats{};
  if (!eng || !st) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bad arguments", who);
  if (!st->series || !st->times)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the state needs TAD_STATE_SERIES | TAD_STATE_TIMES; state unchanged", who);
  if (!bucket_args_ok(bucket_s, bucket_origin))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bucket_s must be >= 1 and 0 <= bucket_origin < bucket_s (got %lld, %lld); state unchanged", who,
                (long long)bucket_s, (long long)bucket_origin);
  if (bucket_op != TAD_OP_SUM && bucket_op != TAD_OP_MAX)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: bucket_op must be TAD_OP_SUM or TAD_OP_MAX; state unchanged", who);
  if (!(ewma_alpha >= 0.0 && ewma_alpha <= 1.0)) return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: ewma_alpha out of range; state unchanged", who);
  constexpr int64_t kLimit = (int64_t)1 << 62;
  if (before_t >= kLimit || before_t <= -kLimit)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: |before_t| must be below 2^62; state unchanged", who);
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "%s: the series was imported without its times (tad_state_import_times)", who);
  const long long b = (long long)bucket_start(before_t, bucket_s, bucket_origin);   // no bucket straddles the bound
  const uint64_t K = st->K;
  const int cur = st->cur, cand = cur ^ 1;
  const uint64_t S = st->ser.len[cur];
  tad_rollup_stats rs{};
  rs.points_before = rs.points_after = S;
  rs.before_t = b;
  if (S == 0) { if (stats) *stats = rs; return TAD_OK; }
  int rc;
  if ((rc = call.enter(who)) != TAD_OK) return rc;
  JobCtx *e = call.e;
  hipStream_t s = e->stream;
  rs.job_context = e->index;
  const double alpha = ewma_alpha == 0.0 ? 0.5 : ewma_alpha;
  // workspace: the per-key and per-chunk arrays of RollupKeys (bk_key) and the scan scratch, held against the limit before anything is written
  const uint64_t bound = trim_chunks_bound(K, S);
  const size_t scan_bytes = scan_scratch_elems(bound > K ? bound : K) * sizeof(unsigned long long);
  const size_t need = carved_bytes(rollup_keys_layout, K, bound) + scan_bytes;
  if (need > e->ws_limit)
    return fail(e, TAD_ERR_GRID_TOO_LARGE, "%s needs %llu bytes of scratch > workspace limit %llu; state unchanged", who, (unsigned long long)need,
                (unsigned long long)e->ws_limit);
  RollupKeys rk;
  if ((rc = carve_buf(e, e->bk_key, &rk, rollup_keys_layout, K, bound)) != TAD_OK || (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK) return rc;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  const Segments &ser = st->ser, &hist = st->hist;
  const long long *t_cur = st->ser_times.p[cur];
  // 1. every key's whole segment in chunks; the heads per chunk under rollup_start; 2. their scan = every chunk's first point afterwards;
  // the candidate series offsets, what every key keeps and loses, the counters; one round trip for the totals
  HIP_TRY(e, hipEventRecord(e->ev[0], s));
  HIP_TRY(e, hipMemsetAsync(rk.rc, 0, sizeof(RollupCounters), s));
  launch_win_bounds(s, K, ser.off[cur], t_cur, 0, 0, 0, nullptr, rk.beg, rk.len, rk.ecnt, rk.chunks);
  launch_scan(s, rk.chunks, rk.coff, K, scratch);
  const BucketSource src{ser.off[cur], ser.val.p[cur], t_cur, rk.beg, rk.len};
  launch_rollup_heads(s, bound, rk.coff, K, src, b, (long long)bucket_s, (long long)bucket_origin, rk.hcnt);
  launch_scan(s, rk.hcnt, rk.hoff, bound, scratch);
  launch_rollup_keys(s, K, ser.off[cur], t_cur, rk.coff, rk.hoff, b, ser.off[cand], rk.rcnt, rk.ecnt, rk.rc);
  HIP_TRY(e, hipGetLastError());
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(e->tail_host);
  HIP_TRY(e, hipMemcpyAsync(tot, rk.hoff + bound, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(tot + 1, rk.rc, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  const uint64_t after = tot[0], rolled = tot[1], buckets = tot[2], changed = tot[3];
  if (after > S || buckets > rolled || S - after != rolled - buckets)
    return fail(e, TAD_ERR_HIP, "%s: %llu points of %llu afterwards, %llu of %llu below the bound; state unchanged", who, (unsigned long long)after,
                (unsigned long long)S, (unsigned long long)buckets, (unsigned long long)rolled);
  if (rolled == 0) { if (stats) *stats = rs; return TAD_OK; }   // nothing below the bound: the state stays as it is (the candidate offsets are scratch)
  // 3. the candidate arenas at their new size (the trim's rule): an allocation failure leaves the state as it is
  if ((rc = size_arenas(e, st, cand, after, after, true, who)) != TAD_OK) return rc;
  // 4. the fold, straight into the candidate values and times; 5. the history: the new values sorted per key; 6. the moments and last_t
  launch_rollup_fold(s, bound, rk.coff, K, src, b, (long long)bucket_s, (long long)bucket_origin, bucket_op == TAD_OP_MAX, rk.hoff, after, ser.val.p[cand],
                     st->ser_times.p[cand]);
  if (st->history) {
    HIP_TRY(e, hipMemcpyAsync(hist.off[cand], ser.off[cand], (K + 1) * 8, hipMemcpyDeviceToDevice, s));
    launch_hist_sort(s, ser.val.p[cand], ser.off[cand], K, hist.val.p[cand], rk.chunks, rk.long_count);   // (chunks: read for the last time by the scan to coff)
  }
  launch_rollup_moments(s, K, rk.rcnt, rk.ecnt, ser.off[cand], ser.val.p[cand], st->ser_times.p[cand], alpha, state_view(st, cur), state_view(st, cand));
  HIP_TRY(e, hipEventRecord(e->ev[1], s));
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(s));
  float ms = 0.f;
  HIP_TRY(e, hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
  // everything succeeded: the candidate becomes current; the old arenas, now the candidates, are given back when far too big for it
  state_commit(st, after, after);
  (void)size_arenas(e, st, cur, after, after, false, who);
  rs.points_after = after;
  rs.points_rolled = rolled;
  rs.buckets = buckets;
  rs.keys_changed = changed;
  rs.ms_total = ms;
  if (stats) *stats = rs;
  return TAD_OK;
}

// tad.h: the unseen and the idle keys leave, the survivors are renumbered densely (kernels in tad_compact.hip).  Fresh moment blocks and
// offsets at the new key count and, when points leave, the candidate arenas are written; they become the state's together once every
// launch has succeeded.
int tad_state_compact(tad_engine *eng, tad_state *st, int64_t retire_before_t, uint64_t *remap, tad_mem remap_memory, tad_compact_stats *stats) {
  if (!eng) return fail(nullptr, TAD_ERR_INVALID_ARGUMENT, "tad_state_compact: engine is NULL");
  if (!st || !remap || (remap_memory != TAD_MEM_HOST && remap_memory != TAD_MEM_DEVICE))
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_compact: bad arguments (state, remap of num_keys entries in host or device memory); state unchanged");
  StateCall call(eng, st);
  if (st->times_stale)
    return fail(eng, TAD_ERR_INVALID_ARGUMENT, "tad_state_compact: the series was imported without its times (tad_state_import_times)");
  const uint64_t K = st->K;
  const int cur = st->cur, cand = cur ^ 1;
  int rc;
  if ((rc = call.enter("tad_state_compact")) != TAD_OK) return rc;
  JobCtx *e = call.e;
  hipStream_t s = e->stream;
  const bool host_remap = remap_memory == TAD_MEM_HOST;
  // workspace: the per-key counts and offsets of CompactKeys (hs_kcnt / hs_koff), the scan scratch; in_key = a host remap's staging
  const size_t scan_bytes = scan_scratch_elems(K) * sizeof(unsigned long long);
  const size_t need = compact_workspace_bytes(K, scan_bytes, host_remap);
  if (need > e->ws_limit)
    return fail(e, TAD_ERR_GRID_TOO_LARGE, "tad_state_compact needs %llu bytes of scratch > workspace limit %llu; state unchanged", (unsigned long long)need,
                (unsigned long long)e->ws_limit);
  CompactKeys ck;
  if ((rc = carve_bufs(e, e->hs_kcnt, e->hs_koff, &ck, compact_keys_layout, K)) != TAD_OK || (rc = ensure(e, e->scan_scratch, scan_bytes)) != TAD_OK ||
      (host_remap && (rc = ensure(e, e->in_key, (size_t)K * 8)) != TAD_OK))
    return rc;
  unsigned long long *scratch = static_cast<unsigned long long *>(e->scan_scratch.p);
  unsigned long long *d_remap = host_remap ? static_cast<unsigned long long *>(e->in_key.p) : reinterpret_cast<unsigned long long *>(remap);
  const StreamState cur_view = state_view(st, cur);
  const Segments &ser = st->ser, &hist = st->hist;
  // 1. who survives, what it keeps; 2. the new ids, the candidate offsets and the chunk offsets; one round trip for the totals
  HIP_TRY(e, hipEventRecord(e->ev[0], s));
  HIP_TRY(e, hipMemsetAsync(ck.cc, 0, sizeof(CompactCounters), s));
  launch_compact_mark(s, K, cur_view, st->series ? ser.off[cur] : nullptr, st->history ? hist.off[cur] : nullptr, (long long)retire_before_t, ck.live,
                      ck.slen, ck.hlen, ck.schunks, ck.hchunks, ck.cc);
  launch_scan(s, ck.live, ck.newid, K, scratch);
  launch_scan(s, ck.slen, ck.sscan, K, scratch);
  launch_scan(s, ck.hlen, ck.hscan, K, scratch);
  launch_scan(s, ck.schunks, ck.scoff, K, scratch);
  launch_scan(s, ck.hchunks, ck.hcoff, K, scratch);
  HIP_TRY(e, hipGetLastError());
  unsigned long long *tot = reinterpret_cast<unsigned long long *>(e->tail_host);
  const unsigned long long *tails[5] = {ck.newid + K, ck.sscan + K, ck.hscan + K, ck.scoff + K, ck.hcoff + K};
  for (int i = 0; i < 5; ++i) HIP_TRY(e, hipMemcpyAsync(tot + i, tails[i], 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipMemcpyAsync(tot + 5, ck.cc, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(e, hipStreamSynchronize(s));
  const uint64_t m = tot[0], skept = tot[1], hkept = tot[2], s_chunks = tot[3], h_chunks = tot[4];
  const uint64_t n_unseen = tot[5], n_idle = tot[6], dropped = tot[7];
  if (m > K || m + n_unseen + n_idle != K) return fail(e, TAD_ERR_HIP, "tad_state_compact: %llu survivors of %llu keys; state unchanged", (unsigned long long)m, (unsigned long long)K);
  tad_compact_stats cs{};
  cs.keys_before = K;
  cs.keys_after = m;
  cs.keys_unseen = n_unseen;
  cs.keys_idle = n_idle;
  cs.points_dropped = dropped;
  cs.bytes_before = state_device_bytes(st);
  cs.job_context = e->index;
  auto remap_out = [&]() -> int {
    if (host_remap) HIP_TRY(e, hipMemcpyAsync(remap, d_remap, K * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipEventRecord(e->ev[1], s));
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipStreamSynchronize(s));
    HIP_TRY(e, hipEventElapsedTime(&cs.ms_total, e->ev[0], e->ev[1]));
    return TAD_OK;
  };
  if (m == K) {   // nothing retired: the identity, the state as it is
    launch_compact_keys(s, K, ck.live, ck.newid, ck.sscan, ck.hscan, false, cur_view, cur_view, nullptr, nullptr, d_remap);
    if ((rc = remap_out()) != TAD_OK) return rc;
    cs.num_keys = K;
    cs.bytes_after = cs.bytes_before;
    if (stats) *stats = cs;
    return TAD_OK;
  }
  // 3. fresh moment blocks and offsets for max(m, 1) keys, all zero: with no survivor the one key left is unseen and its segments empty
  // (the old ones stay the state's until everything succeeded)
  const uint64_t Km = m ? m : 1;
  const bool gather = dropped != 0;        // only unseen keys went: the arenas already are the survivors' segments in order
  const int to = gather ? cand : cur;      // the copy that is current afterwards
  tad_state fresh;
  fresh.K = Km;
  fresh.history = st->history;
  fresh.series = st->series;
  hipError_t r = alloc_keyed(&fresh, Km, s);
  auto drop_fresh = [&]() {
    (void)hipStreamSynchronize(s);
    free_keyed(&fresh);
  };
  if (r != hipSuccess) {
    (void)hipGetLastError();
    drop_fresh();
    return fail(e, TAD_ERR_OUT_OF_MEMORY, "tad_state_compact: %s (state unchanged)", hipGetErrorString(r));
  }
  // the candidate arenas at their new size (the trim's rule): an allocation failure leaves the state as it is
  if (gather && (rc = size_arenas(e, st, cand, skept, hkept, true, "tad_state_compact")) != TAD_OK) { drop_fresh(); return rc; }
  // 4. the survivors' moments and offsets, remap; 5. their segments
  launch_compact_keys(s, K, ck.live, ck.newid, ck.sscan, ck.hscan, true, cur_view, stream_view(fresh.block[to], Km), st->series ? fresh.ser.off[to] : nullptr,
                      st->history ? fresh.hist.off[to] : nullptr, d_remap);
  if (gather && st->series)
    launch_compact_copy(s, s_chunks, ck.scoff, K, ser.off[cur], ser.val.p[cur], st->times ? st->ser_times.p[cur] : nullptr, ck.sscan, ser.val.p[cand],
                        st->times ? st->ser_times.p[cand] : nullptr);
  if (gather && st->history) launch_compact_copy(s, h_chunks, ck.hcoff, K, hist.off[cur], hist.val.p[cur], nullptr, ck.hscan, hist.val.p[cand], nullptr);
  if ((rc = remap_out()) != TAD_OK) { drop_fresh(); return rc; }
  // everything succeeded: the fresh blocks and offsets replace the old ones; after a gather the candidate arenas become current and the
  // old ones, now the candidates, are given back when far too big
  adopt_keyed(st, &fresh);
  if (gather) {
    state_commit(st, skept, hkept);
    (void)size_arenas(e, st, cur, skept, hkept, false, "tad_state_compact");
    cs.series_points_moved = st->series ? skept : 0;
    cs.history_points_moved = st->history ? hkept : 0;
  }
  cs.num_keys = Km;
  cs.bytes_after = state_device_bytes(st);
  if (stats) *stats = cs;
  return TAD_OK;
}

}  // extern "C"
