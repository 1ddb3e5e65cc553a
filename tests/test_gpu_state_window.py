"""GPU: the batch verdicts over a window of a streaming state (tad_run_state_window, include/tad.h).  The defining property: let W be the
table with one row per series point the state holds and W' its rows inside the window — flow_end_s >= from_t, < to_t, then the newest
keep_points of every key; the call returns exactly the rows tad_run returns for W' with the same algorithm, parameters and emit flag,
bit for bit, and leaves the state as it was.  Two references: (R1) the engine's own tad_run on W', W' filtered on the host from
export_series / export_times; (R2) oracle.tad_oracle.run_job on W', which is independent of the engine.  Float columns are compared as
uint64 bit patterns.  The helpers follow tests/test_gpu_state_run.py (copied, not imported)."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import arima_oracle as ao
from oracle import tad_oracle as orc
from theia_amd import TadError, _capi
from state_helpers import (ALL, COUNTERS, HIST, ROW_FIELDS, SER, TIMES, T_BASE, assert_rows, assert_same, in_window, minute_batches, new_state,
                           rows_of, second_batches, snapshot, window)

pytestmark = pytest.mark.gpu

ALGOS = ("EWMA", "DBSCAN", "ARIMA")


def coverage(k, m):
    """keys of W by what the window does to them: (cut at the front, cut at the back, wholly inside, wholly outside)"""
    keys, first, n = np.unique(k, return_index=True, return_counts=True)
    n_in = np.add.reduceat(m.astype(np.int64), first)
    last = first + n - 1
    some = (n_in > 0) & (n_in < n)
    return int((some & ~m[first]).sum()), int((some & ~m[last]).sum()), int((n_in == n).sum()), int((n_in == 0).sum())


def r1(engine, K, W, m, algo, emit_all=False, **kw):
    """the engine's own tad_run on W'"""
    k, t, v = W
    return engine.run(algo, k[m], t[m], v[m], K, agg_flow="svc", value_op="sum", emit_all=emit_all, **kw)


def r2_rows(W, m, algo, emit_all=False, maxiter=0, **kw):
    """the oracle's job on W': the rows the engine must return"""
    k, t, v = W
    if algo == "ARIMA" and maxiter:
        kw["arima_fn"] = lambda x, counters=None: ao.calculate_arima_exact(x, maxiter=maxiter, counters=counters)
    want = orc.run_job(algo, k[m], t[m], v[m], op="sum", **kw)
    if not emit_all:
        return {f: want[f] for f in ROW_FIELDS}
    pk, pt, pv = want["points"]
    sel = np.ones(pk.size, bool)
    if algo == "ARIMA":                                       # keys with no result emit nothing
        sel = np.repeat(np.array([r is not None for r in want["arima_results"]], bool), np.diff(want["ptr"]))
    sig = np.repeat(want["sigma"], np.diff(want["ptr"]))
    return {"key_id": pk[sel], "flow_end_s": pt[sel], "throughput": orc.u64_to_f64(pv)[sel], "algo_calc": want["calc_all"][sel],
            "stddev": sig[sel], "anomaly": want["anomaly_all"][sel].astype(np.uint8)}


def check(engine, st, W, win, algo, emit_all=False, what="", oracle=True, snap=None, **kw):
    """run_state_window equals R1 (rows and counters) and R2 (rows) and leaves the state as it was; returns (result, mask of W')"""
    from_t, to_t, keep = win
    m = in_window(W[0], W[1], from_t, to_t, keep)
    Pw = int(m.sum())
    snap = snap or snapshot(st)
    got = engine.run_state_window(st, from_t, to_t, keep, algo=algo, emit_all=emit_all, **kw)
    assert_same(snapshot(st), snap, (what, win, algo, "state changed"))
    gs = got.stats
    assert gs["rows_in"] == gs["rows_used"] == gs["n_points"] == Pw, (what, win, algo, gs["n_points"], Pw)
    assert (gs["stage0_path"], gs["stage0_attempts"], gs["step"], gs["n_buckets"]) == (0, 0, 0, 0)
    assert gs["ms_meta"] == gs["ms_stage0"] == gs["ms_scatter"] == 0.0
    if Pw == 0:
        assert got.n_rows == 0 and gs["n_keys"] == 0 and gs["t0"] == 0 and gs["n_anomalies"] == 0, (what, win, algo)
        return got, m
    want = r1(engine, st.num_keys, W, m, algo, emit_all, **kw)
    assert_rows(rows_of(got), rows_of(want), (what, win, algo, emit_all, "R1"))
    ws = want.stats
    print("%s %s %s emit_all=%d: window %d of %d points, rows %d, R1 %s" % (what, win, algo, emit_all, Pw, W[0].size, got.n_rows,
                                                                          {f: ws[f] for f in COUNTERS + ("t0",)}))
    for f in COUNTERS + ("t0",):
        assert gs[f] == ws[f], (what, win, algo, f, gs[f], ws[f])
    assert gs["t0"] == int(W[1][m].min())
    if not emit_all:
        assert 0 < got.n_rows < Pw, (what, win, algo, got.n_rows, Pw)            # mixed verdicts: no comparison is vacuous
    if algo == "ARIMA":
        assert gs["arima_fits"] > 0, (what, win)
    if oracle:
        assert_rows(rows_of(got), r2_rows(W, m, algo, emit_all, **kw), (what, win, algo, emit_all, "R2"))
    return got, m


# ---- the shapes ----


MIN = 60
SEC_WIDTH = 3600
# name -> (number of keys for EWMA / DBSCAN, for ARIMA, whose fits are the job's cost): the same generator, fewer keys
SHAPE_KEYS = {"minute": (300, 40), "second": (1500, 90), "long": (503, 503), "merged": (300, 40), "trimmed": (300, 40)}


def build_state(engine, shape, K):
    """one of the five states of the issue; returns (state, extra detector parameters)"""
    st = new_state(engine, K)
    if shape == "minute":                                     # dense minute lattice, 48 buckets
        for bk, bt, bv in minute_batches(200 * K, K, 48, (8, 16, 24, 32, 40)):
            engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
    elif shape == "second":                                   # sparse second resolution, a third of the keys early only, a third late only
        for bk, bt, bv in second_batches(K, 6, SEC_WIDTH, 4, seed=23, lifetimes=True):
            engine.run_stream(st, bk, bt, bv, value_op="max")
    elif shape == "long":                                     # keys 0..2 of about 2900 points, 500 short ones behind them
        k, t, v = orc.synth_rows(0, 30000, 3, 3000)
        sk, stt, sv = orc.synth_rows(0, 20000, 500, 48)
        k, t, v = np.concatenate([k, sk + np.uint64(3)]), np.concatenate([t, stt]), np.concatenate([v, sv])
        edges = [T_BASE + MIN * b for b in (0, 20, 48, 1500, 3000)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            sel = (t >= lo) & (t < hi)
            engine.run_stream(st, k[sel], t[sel], v[sel], value_op="max")
    elif shape == "merged":                                   # out-of-order batches, rows of one group split over batches
        k, t, v = orc.synth_rows(0, 200 * K, K, 48)
        part = np.random.default_rng(5).integers(0, 5, size=k.size)
        for p in (3, 0, 4, 1, 2):
            engine.merge_stream(st, k[part == p], t[part == p], v[part == p], agg_flow="svc", value_op="sum")
    elif shape == "trimmed":                                  # a state after a trim by time and one by count
        for bk, bt, bv in minute_batches(200 * K, K, 60, (15, 30, 45)):
            engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
        st.trim(keep_from=T_BASE + 12 * MIN)
        st.trim(keep_points=44)
    else:
        raise ValueError(shape)
    return st


def shape_windows(shape, W):
    """the nine windows of the issue as (name, (from_t, to_t, keep_points)), chosen from the shape's known time range"""
    t = W[1]
    lo, hi = int(t.min()), int(t.max())
    span = hi - lo
    a, b = lo + span // 4, lo + (3 * span) // 4
    if shape == "second":                                     # (see test_lifetimes_windows_cover_every_kind_of_key)
        a, b = T_BASE + 600, T_BASE + 4 * SEC_WIDTH + 1800
    some = np.sort(np.unique(t))
    ta = int(some[np.searchsorted(some, a)])                  # times that points do have, near a and b
    tb = int(some[np.searchsorted(some, b)])
    keep = {"long": 600, "second": 12}.get(shape, 14)                # (12: the early-only keys' point count, so a count leaves keys whole)
    return [("old end", (a, 0, 0)), ("new end", (0, b, 0)), ("interior", (a, b, 0)), ("interior with count", (a, b, keep)),
            ("count only", (0, 0, keep)), ("empty", (hi + 1, 0, 0)), ("from_t on a point", (ta, 0, 0)), ("to_t on a point", (0, tb, 0)),
            ("whole", (0, 0, 0))]


# On the lifetimes shape, per window: which of (cut at the front, cut at the back, wholly inside, wholly outside) it must produce at
# least once (1) and which it cannot produce at all (0).  A window with one bound cuts one end only; the early-only keys have points
# from the first batch on, so no key lies wholly before a from_t inside that batch; the late-only keys start in batch 4, where some of
# them have every point of that batch after to_t = batch 4 + 1800 s: wholly outside; they hold 8 points and the early-only keys 12, so a count of 12 keeps both whole.
KINDS = ("cut front", "cut back", "inside", "outside")
LIFETIME_KINDS = {"old end": (1, 0, 1, 0), "from_t on a point": (1, 0, 1, 0), "new end": (0, 1, 1, 1), "to_t on a point": (0, 1, 1, 1),
                  "interior": (1, 1, 1, 1), "interior with count": (1, 1, 1, 1), "count only": (1, 0, 1, 0), "empty": (0, 0, 0, 1),
                  "whole": (0, 0, 1, 0)}


def algo_params(shape, algo):
    return {"maxiter": 2} if (shape == "long" and algo == "ARIMA") else {}     # (a fit over 2900 points is the job's cost, not the window's)


# ---- 1. the defining property: every state, every window, every detector ----
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("shape", sorted(SHAPE_KEYS))
def test_window_equals_the_batch_job_on_the_window(engine, shape, algo):
    K = SHAPE_KEYS[shape][algo == "ARIMA"]
    st = build_state(engine, shape, K)
    W = window(st)
    snap = snapshot(st)
    seen_cut = 0
    for name, win in shape_windows(shape, W):
        m = in_window(W[0], W[1], *win)
        cov = coverage(W[0], m)
        cf, cb = cov[:2]
        seen_cut += cf + cb
        if shape == "second":                                 # the lifetimes shape: every kind of key the window CAN make, it makes
            print(shape, name, win, "cut front / cut back / inside / outside:", cov)
            for kind, n, must in zip(KINDS, cov, LIFETIME_KINDS[name]):
                assert (n >= 1) if must else (n == 0), (name, kind, cov)
        if name == "from_t on a point":                       # inclusive: the point at from_t is inside
            assert m[W[1] == win[0]].all() and (W[1] == win[0]).any()
        if name == "to_t on a point":                         # exclusive: the point at to_t is outside
            assert not m[W[1] == win[1]].any() and (W[1] == win[1]).any()
        if name == "empty":
            assert not m.any()
        if name == "whole":
            assert m.all()
        for emit_all in (False, True):
            check(engine, st, W, win, algo, emit_all, what=(shape, name), snap=snap, **algo_params(shape, algo))
    assert seen_cut > 0
    st.close()


# ---- 2. not vacuous: what the windows do to the keys of the lifetimes shape ----
LIFETIME_WINDOWS = [("interior", (T_BASE + 600, T_BASE + 4 * SEC_WIDTH + 1800, 0)),
                    ("interior with count", (T_BASE + 600, T_BASE + 4 * SEC_WIDTH + 1800, 12)),
                    ("interior, other bounds", (T_BASE + 300, T_BASE + 4 * SEC_WIDTH + 900, 0)),
                    ("interior on points", None)]


def lifetime_points(K):
    """W of the lifetimes shape on the host: the distinct (key, time) points of its batches, values by max"""
    cat = [np.concatenate(c) for c in zip(*second_batches(K, 6, SEC_WIDTH, 4, seed=23, lifetimes=True))]
    return orc.stage0(cat[0], cat[1], cat[2], "max")


def lifetime_window(name, win, W):
    if win is not None:
        return win
    some = np.sort(np.unique(W[1]))                           # both bounds equal to times that points have
    return (int(some[np.searchsorted(some, T_BASE + 600)]), int(some[np.searchsorted(some, T_BASE + 4 * SEC_WIDTH + 1800)]), 0)


@pytest.mark.parametrize("name,win", LIFETIME_WINDOWS, ids=[n for n, _ in LIFETIME_WINDOWS])
def test_lifetimes_windows_cover_every_kind_of_key(engine, name, win):
    """On the lifetimes shape every window here cuts keys at the front, cuts keys at the back, keeps keys whole and leaves keys out —
    asserted from W and W' on the host before the device is asked.  (A window with one bound cannot cut at the other end: those run in
    test_window_equals_the_batch_job_on_the_window, which asserts the kinds of key each of them can make: LIFETIME_KINDS.)"""
    K = SHAPE_KEYS["second"][0]
    W = lifetime_points(K)
    win = lifetime_window(name, win, W)
    m = in_window(W[0], W[1], *win)
    cov = coverage(W[0], m)
    print(name, win, "cut front / cut back / inside / outside:", cov)
    assert min(cov) >= 1, cov
    st = build_state(engine, "second", K)
    Ws = window(st)
    assert all(np.array_equal(x, y) for x, y in zip(Ws, W))   # the state holds the generator's points
    for algo in ("EWMA", "DBSCAN"):
        for emit_all in (False, True):
            check(engine, st, Ws, win, algo, emit_all, what=name)
    st.close()
    Ka = SHAPE_KEYS["second"][1]
    Wa = lifetime_points(Ka)
    assert min(coverage(Wa[0], in_window(Wa[0], Wa[1], *lifetime_window(name, win, Wa)))) >= 1
    st = build_state(engine, "second", Ka)
    for emit_all in (False, True):
        check(engine, st, window(st), lifetime_window(name, win, Wa), "ARIMA", emit_all, what=name)
    st.close()


# ---- 3. to_t == 0: the rows of run_state on a trimmed copy ----
@pytest.mark.parametrize("shape", ("minute", "second", "long"))
def test_equals_run_state_after_a_trim(engine, shape):
    K = SHAPE_KEYS[shape][0]
    st = build_state(engine, shape, K)
    snap = snapshot(st)
    W = window(st)
    lo, hi = int(W[1].min()), int(W[1].max())
    for keep, from_t in ((0, lo + (hi - lo) // 3), (7, 0), (5, lo + (hi - lo) // 2), (0, hi + 1)):
        cp = new_state(engine, K)
        cp.load(snap["state"])
        cp.load_history(*snap["history"])
        cp.load_series(*snap["series"])
        cp.load_times(snap["times"])
        cp.trim(keep_points=keep, keep_from=from_t)
        for algo in ALGOS if shape == "minute" else ("EWMA", "DBSCAN"):
            kw = {"maxiter": 3} if algo == "ARIMA" else {}
            for emit_all in (False, True):
                a = engine.run_state_window(st, from_t, 0, keep, algo=algo, emit_all=emit_all, **kw)
                b = engine.run_state(cp, algo=algo, emit_all=emit_all, **kw)
                assert_rows(rows_of(a), rows_of(b), (shape, keep, from_t, algo, emit_all))
                for f in COUNTERS + ("t0",):
                    assert a.stats[f] == b.stats[f], (shape, keep, from_t, algo, f)
        assert_same(snapshot(st), snap)
        cp.close()
    st.close()


# ---- 4. the whole state ----
def test_zero_window_is_run_state(engine):
    K = 200
    st = build_state(engine, "minute", K)
    W = window(st)
    for algo in ALGOS:
        kw = {"maxiter": 3} if algo == "ARIMA" else {}
        for emit_all in (False, True):
            a = engine.run_state_window(st, algo=algo, emit_all=emit_all, **kw)
            b = engine.run_state(st, algo=algo, emit_all=emit_all, **kw)
            assert a.n_rows > 0
            assert_rows(rows_of(a), rows_of(b), (algo, emit_all))
            for f in COUNTERS + ("t0", "rows_in", "rows_used", "pts_mean", "pts_m2"):
                assert a.stats[f] == b.stats[f], (algo, f)
            # bounds that leave every key whole take the same path: the state's own arrays
            c = engine.run_state_window(st, int(W[1].min()), int(W[1].max()) + 1, 1000, algo=algo, emit_all=emit_all, **kw)
            assert_rows(rows_of(c), rows_of(b), (algo, emit_all, "wide bounds"))
    st.close()


# ---- 5. DBSCAN's window history: sorted from the window, or the state's history without the excluded values ----
def test_both_history_paths(engine):
    """the rule (tad.h): 2 * (window points) <= (state points) sorts the window's values; otherwise the excluded values are sorted and
    subtracted from the state's history"""
    for shape in ("minute", "second", "long"):
        st = build_state(engine, shape, SHAPE_KEYS[shape][0])
        W = window(st)
        S = W[0].size
        lo, hi = int(W[1].min()), int(W[1].max())
        small = (lo + (hi - lo) * 7 // 10, 0, 0)              # the newest three tenths
        if shape == "long":                                   # (the short keys, which have the noise, end after 48 minutes: their first half)
            small = (0, lo + 24 * MIN, 0)
        large = (0, hi - (hi - lo) // 10, 0)                  # all but the newest tenth
        both = (lo + (hi - lo) // 10, hi - (hi - lo) // 10, 0)   # a prefix and a suffix excluded
        if shape == "long":
            both = (lo + 5 * MIN, hi - (hi - lo) // 10, 0)
        for win, by_sort in ((small, True), (large, False), (both, False)):
            Pw = int(in_window(W[0], W[1], *win).sum())
            assert 0 < Pw < S and (2 * Pw <= S) == by_sort, (shape, win, Pw, S)
            assert bool(engine._lib.tad_window_history_by_sort(Pw, S)) == by_sort      # the library decides as the host expects
            for emit_all in (False, True):
                check(engine, st, W, win, "DBSCAN", emit_all, what=(shape, "sort" if by_sort else "subtract"))
                if shape == "minute":
                    check(engine, st, W, win, "DBSCAN", emit_all, what=(shape, "eps"), eps=9.0e7, min_samples=6)
        st.close()


# ---- 6. refusals leave the state unchanged ----
def raw_call(engine, st, from_t=0, to_t=0, keep=0, **job):
    j = _capi.Job(**job)
    res = C.POINTER(_capi.Result)()
    rc = engine._lib.tad_run_state_window(engine._h, st._h, C.byref(j), from_t, to_t, keep, _capi.TAD_MEM_HOST, C.byref(res))
    if rc == _capi.TAD_OK:
        engine._lib.tad_result_free(engine._h, res)
    else:
        assert not res
    return rc


def test_refusals(engine):
    K = 50
    batches = minute_batches(12000, K, 30, (15,))
    a, b = T_BASE + 5 * MIN, T_BASE + 20 * MIN
    for flags in (0, HIST, SER, HIST | SER, SER | TIMES, ALL):     # plain, history only, series without times (with and without history), ...
        st = new_state(engine, K, flags)
        for bk, bt, bv in batches:
            engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
        snap = snapshot(st)
        for algo in ("EWMA", "DBSCAN", "ARIMA", "DROP"):
            ok = algo != "DROP" and (flags & (SER | TIMES)) == (SER | TIMES) and (algo != "DBSCAN" or flags & HIST)
            if ok:
                assert engine.run_state_window(st, a, b, algo=algo, emit_all=True).n_rows > 0
            else:
                with pytest.raises(TadError) as ei:
                    engine.run_state_window(st, a, b, algo=algo)
                assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT, (flags, algo)
            assert_same(snapshot(st), snap, (flags, algo))
        if flags == ALL:
            assert raw_call(engine, st, a, b, algo=0) == _capi.TAD_OK
            assert raw_call(engine, st, a, a, algo=0) == _capi.TAD_OK                      # from_t == to_t: an empty window
            assert engine.run_state_window(st, a, a).n_rows == 0
            assert raw_call(engine, st, b, a, algo=0) == _capi.TAD_ERR_INVALID_ARGUMENT   # from_t > to_t
            assert_same(snapshot(st), snap, "from_t > to_t")
            for bad in (dict(start_time=T_BASE), dict(end_time=T_BASE + 600), dict(start_time=T_BASE, end_time=T_BASE + 600),
                        dict(flags=_capi.TAD_FLAG_KEY_U32), dict(flags=_capi.TAD_FLAG_TIME_U32), dict(ewma_alpha=1.5)):
                assert raw_call(engine, st, a, b, algo=0, **bad) == _capi.TAD_ERR_INVALID_ARGUMENT, bad
                assert_same(snapshot(st), snap, bad)
            stale = new_state(engine, K)                      # the series imported, its times not yet
            stale.load(snap["state"])
            stale.load_history(*snap["history"])
            stale.load_series(*snap["series"])
            with pytest.raises(TadError) as ei:
                engine.run_state_window(stale, a, b)
            assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT
            assert np.array_equal(stale.export_series()[1], snap["series"][1])
            stale.load_times(snap["times"])
            assert_rows(rows_of(engine.run_state_window(stale, a, b)), rows_of(engine.run_state_window(st, a, b)), "times imported")
            stale.close()
        assert_same(snapshot(st), snap, flags)
        st.close()
    st = new_state(engine, K)                                 # an empty state: no rows, no error
    for algo in ALGOS:
        for emit_all in (False, True):
            r = engine.run_state_window(st, a, b, 3, algo=algo, emit_all=emit_all)
            assert r.n_rows == 0 and r.stats["n_points"] == 0 and r.stats["n_keys"] == 0 and r.stats["t0"] == 0
    st.close()


# ---- 7. concurrency ----
def test_two_threads_on_two_states_and_beside_a_job(engine):
    K = 200
    states = [build_state(engine, "minute", K), build_state(engine, "merged", K)]
    wins = [(T_BASE + 10 * MIN, T_BASE + 40 * MIN, 0), (0, T_BASE + 30 * MIN, 12)]
    algos = ("EWMA", "DBSCAN")
    serial = [rows_of(engine.run_state_window(st, *win, algo=algo, emit_all=True)) for st, win, algo in zip(states, wins, algos)]
    jk, jt, jv = orc.synth_rows(1, 1 << 18, 2000, 60)
    job_serial = rows_of(engine.run("EWMA", jk, jt, jv, 2000, agg_flow="svc"))
    snaps = [snapshot(st) for st in states]
    errors = []

    def worker(i):
        try:
            for n in range(15):
                got = engine.run_state_window(states[i], *wins[i], algo=algos[i], emit_all=True, job_id="w%d-%d" % (i, n))
                assert_rows(rows_of(got), serial[i], (i, n))
        except Exception as exc:      # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    def job():
        try:
            for n in range(6):
                assert_rows(rows_of(engine.run("EWMA", jk, jt, jv, 2000, agg_flow="svc")), job_serial, ("job", n))
        except Exception as exc:      # noqa: BLE001
            errors.append(exc)

    for targets in ([lambda: worker(0), lambda: worker(1)], [lambda: worker(0), job]):
        threads = [threading.Thread(target=f) for f in targets]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
    assert engine.jobs_in_flight() == 0
    for st, snap in zip(states, snaps):
        assert_same(snapshot(st), snap)
        st.close()


# ---- 8. device results ----
def test_device_results(engine):
    st = build_state(engine, "minute", 120)
    win = (T_BASE + 9 * MIN, T_BASE + 41 * MIN, 20)
    for algo in ALGOS:
        kw = {"maxiter": 3} if algo == "ARIMA" else {}
        for emit_all in (False, True):
            host = engine.run_state_window(st, *win, algo=algo, emit_all=emit_all, job_id="w-%s" % algo, **kw)
            dev = engine.run_state_window(st, *win, algo=algo, emit_all=emit_all, out="device", job_id="w-%s" % algo, **kw)
            assert dev.memory == "device" and host.id == dev.id == "w-%s" % algo and host.n_rows > 0
            assert_rows(rows_of(dev), rows_of(host), (algo, emit_all, "device"))
            assert dev.stats["n_anomalies"] == host.stats["n_anomalies"]
            dev.close()
    st.close()
