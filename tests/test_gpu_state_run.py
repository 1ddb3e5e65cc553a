"""GPU: the batch verdicts of a streaming state's whole window (tad_run_state, include/tad.h).  The defining property: let W be the table
with one row per series point the state holds; tad_run_state returns exactly the rows tad_run returns for W with the same algorithm,
parameters and emit flag — key, time, throughput, algo_calc, stddev (and the verdicts with emit_all) in the same order, bit for bit —
and leaves the state as it was.  Two references: (R1) the engine's own tad_run on W, W taken from export_series / export_times;
(R2) oracle.tad_oracle.run_job on W, which is independent of the engine.  Float columns are compared as uint64 bit patterns."""
import threading

import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadError, _capi
from state_helpers import (ALL, HIST, ROW_FIELDS, SER, TIMES, T_BASE, assert_rows, assert_same, bits, minute_batches, new_state, raw_run_state,
                           rows_of, second_batches, snapshot, window)

pytestmark = pytest.mark.gpu


def r1(engine, st, algo, emit_all=False, **kw):
    """the engine's own tad_run on W"""
    k, t, v = window(st)
    return engine.run(algo, k, t, v, st.num_keys, agg_flow="svc", value_op="sum", emit_all=emit_all, **kw)


def r2(st, algo, **kw):
    """the oracle's job on W"""
    k, t, v = window(st)
    return orc.run_job(algo, k, t, v, op="sum", **kw)


def check(engine, st, algo, emit_all=False, what="", **kw):
    """run_state equals R1, rows and counters, and leaves the state as it was; returns (result, R1's result)"""
    snap = snapshot(st)
    got = engine.run_state(st, algo=algo, emit_all=emit_all, **kw)
    assert_same(snapshot(st), snap, (what, algo, "state changed"))
    want = r1(engine, st, algo, emit_all, **kw)
    assert_rows(rows_of(got), rows_of(want), (what, algo, emit_all))
    gs, ws = got.stats, want.stats
    P = st.series_points()
    assert gs["rows_in"] == gs["rows_used"] == gs["n_points"] == P == ws["n_points"], (what, algo)
    for f in ("n_keys", "n_anomalies", "keys_no_result", "arima_fits", "arima_nan_fits", "kalman_steps"):
        assert gs[f] == ws[f], (what, algo, f, gs[f], ws[f])
    assert (gs["stage0_path"], gs["stage0_attempts"], gs["step"], gs["n_buckets"]) == (0, 0, 0, 0)
    assert gs["ms_meta"] == gs["ms_stage0"] == gs["ms_scatter"] == 0.0
    assert gs["t0"] == (int(window(st)[1].min()) if P else 0)
    return got, want


def check_oracle(engine, st, algo, what="", **kw):
    got = engine.run_state(st, algo=algo, **kw)
    want = r2(st, algo, **kw)
    assert_rows(rows_of(got), {f: want[f] for f in ROW_FIELDS}, (what, algo, "oracle"))
    assert got.stats["n_anomalies"] == want["n_anomalies"] and got.stats["n_keys"] == want["n_keys"] and got.stats["n_points"] == want["n_points"]
    return got, want


# ---- 1. minute lattice, sum ----
def test_minute_lattice_after_every_batch_and_after_trims(engine):
    K = 300
    batches = minute_batches(60000, K, 48, (8, 16, 24, 32, 40))
    st = new_state(engine, K)
    for b, (bk, bt, bv) in enumerate(batches):
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
        for algo in ("EWMA", "DBSCAN"):
            for emit_all in (False, True):
                got, _ = check(engine, st, algo, emit_all, what=b)
                assert 0 < got.stats["n_anomalies"] < got.stats["n_points"]      # mixed verdicts: no comparison is vacuous
    st.trim(keep_from=T_BASE + 24 * 60)
    counts = {}
    for algo in ("EWMA", "DBSCAN"):
        for emit_all in (False, True):
            check(engine, st, algo, emit_all, what="trimmed")
        got, _ = check_oracle(engine, st, algo, what="trimmed")
        counts[algo] = got.stats["n_anomalies"]
        assert (got.stats["n_points"], got.stats["n_keys"]) == (7096, 300)
        gm = orc.u64_to_f64(window(st)[2]).mean()
        assert abs(got.stats["pts_mean"] - gm) <= 1e-12 * gm
    assert counts == {"EWMA": 787, "DBSCAN": 2696}, counts
    st.trim(keep_points=9)
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False, what="keep_points")
        check(engine, st, algo, True, what="keep_points")
        check_oracle(engine, st, algo, what="keep_points")
    st.close()


# ---- 2. short and one-point keys, max ----
def test_short_and_one_point_keys(engine):
    K = 2000
    batches = minute_batches(20000, K, 48, (8, 16, 24, 32, 40))
    st = new_state(engine, K)
    for bk, bt, bv in batches:
        engine.run_stream(st, bk, bt, bv, value_op="max")
    before = st.export()["n"]
    st.trim(keep_from=T_BASE + 40 * 60)
    n = st.export()["n"]
    assert ((before > 0) & (n == 0)).any() and (n == 1).sum() == 715     # keys emptied by the trim; one-point keys
    counts = {}
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False)
        got_all, _ = check(engine, st, algo, True)
        got, _ = check_oracle(engine, st, algo)
        assert (got.stats["n_points"], got.stats["n_keys"]) == (3004, 1624)
        counts[algo] = got.stats["n_anomalies"]
        one = n[got_all["key_id"].astype(np.int64)] == 1
        assert one.sum() == 715 and (got_all["stddev"][one] == 0.0).all()
        if algo == "EWMA":
            assert not got_all["anomaly"][one].any()                     # no sigma, no verdict
        else:
            assert got_all["anomaly"][one].all()                         # fewer than min_samples points: noise
    assert counts == {"EWMA": 2289, "DBSCAN": 2580}, counts
    st.close()


# ---- 3. long keys: the wavefront-per-key walk ----
def long_rows():
    return orc.synth_rows(0, 30000, 3, 3000)


def stream_in_batches(engine, st, k, t, v, edges, op):
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (t >= lo) & (t < hi)
        if sel.any():
            engine.run_stream(st, k[sel], t[sel], v[sel], value_op=op)


def test_long_keys(engine):
    k, t, v = long_rows()
    st = new_state(engine, 3)
    stream_in_batches(engine, st, k, t, v, [T_BASE + 60 * b for b in (0, 700, 1900, 3000)], "max")     # (the counts below are the oracle's for `max`)
    n = st.export()["n"]
    assert n.min() >= 2885 and n.max() <= 2906, n
    counts = {}
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False)
        check(engine, st, algo, True)
        counts[algo] = check_oracle(engine, st, algo)[0].stats["n_anomalies"]
    assert counts == {"EWMA": 284, "DBSCAN": 4}, counts
    st.close()


def test_long_keys_among_short_ones(engine):
    K = 503                                                  # keys 0..2 long, 500 short ones behind them
    k, t, v = long_rows()
    sk, stt, sv = orc.synth_rows(0, 20000, 500, 48)
    k, t, v = np.concatenate([k, sk + np.uint64(3)]), np.concatenate([t, stt]), np.concatenate([v, sv])
    st = new_state(engine, K)
    stream_in_batches(engine, st, k, t, v, [T_BASE + 60 * b for b in (0, 20, 48, 1500, 3000)], "max")
    n = st.export()["n"]
    assert n[:3].min() >= 2885 and 0 < n[3:].max() <= 48
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False)
        check(engine, st, algo, True)
        check_oracle(engine, st, algo)
    st.resize(9000)                                          # many keys, most of them unseen: the long ones are outliers of the launch
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False, what="resized")
        check(engine, st, algo, True, what="resized")
    st.trim(keep_points=600)                                 # the long keys still take a wavefront each, at another length
    for algo in ("EWMA", "DBSCAN"):
        check(engine, st, algo, False, what="resized, trimmed")
        check_oracle(engine, st, algo, what="resized, trimmed")
    st.close()


# ---- 4. second-resolution connection keys through the sparse stream path ----
def test_second_resolution_keys_with_trims_between_batches(engine):
    K, width = 5000, 3600
    batches = second_batches(K, 6, width, 3, seed=17, lifetimes=True)
    st = new_state(engine, K)
    for b, (bk, bt, bv) in enumerate(batches):
        if b >= 2:
            st.trim(keep_from=T_BASE + (b - 2) * width + 1200)
        r = engine.run_stream(st, bk, bt, bv, value_op="max")
        assert r.stats["stage0_path"] in (4, 8), r.stats["stage0_path"]
        for algo in ("EWMA", "DBSCAN"):
            check(engine, st, algo, b % 2 == 0, what=b)
    n = st.export()["n"]
    assert (n == 0).any() and n.max() > 3                    # keys the trims emptied beside keys alive throughout
    for algo in ("EWMA", "DBSCAN"):
        check_oracle(engine, st, algo)
    st.close()


# ---- 5. parameters; device results ----
def test_parameters_and_device_results(engine):
    K = 120
    st = new_state(engine, K)
    for bk, bt, bv in minute_batches(30000, K, 60, (20, 45)):
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum", alpha=0.5)
    a, _ = check(engine, st, "EWMA", True, alpha=0.3)        # the state's stored ewma (alpha 0.5) is not used
    b, _ = check(engine, st, "EWMA", True)
    assert not np.array_equal(bits(a["algo_calc"]), bits(b["algo_calc"]))
    want = r2(st, "EWMA", alpha=0.3)
    assert_rows(rows_of(engine.run_state(st, alpha=0.3)), {f: want[f] for f in ROW_FIELDS}, "alpha")
    c, _ = check(engine, st, "DBSCAN", True, eps=9.0e7, min_samples=6)
    d, _ = check(engine, st, "DBSCAN", True)
    assert c.stats["n_anomalies"] != d.stats["n_anomalies"]
    want = r2(st, "DBSCAN", eps=9.0e7, min_samples=6)
    assert_rows(rows_of(engine.run_state(st, algo="DBSCAN", eps=9.0e7, min_samples=6)), {f: want[f] for f in ROW_FIELDS}, "eps")
    for algo in ("EWMA", "DBSCAN"):
        for emit_all in (False, True):
            host = engine.run_state(st, algo=algo, emit_all=emit_all, job_id="w-%s" % algo)
            dev = engine.run_state(st, algo=algo, emit_all=emit_all, out="device", job_id="w-%s" % algo)
            assert dev.memory == "device" and host.id == dev.id == "w-%s" % algo
            assert_rows(rows_of(dev), rows_of(host), (algo, emit_all, "device"))
            assert dev.stats["n_anomalies"] == host.stats["n_anomalies"]
            dev.close()
    st.close()


def test_ewma_emit_variants(engine):
    """the LDS-staged emit, the same with a capacity far below a wavefront's rows (the rest is stored directly) and the lane-per-key
    emit give the same rows"""
    K = 700
    st = new_state(engine, K)
    for bk, bt, bv in minute_batches(150000, K, 120, (40, 80)):
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
    want = rows_of(r1(engine, st, "EWMA"))
    assert want["key_id"].size > 64 * (K // 64)               # more rows than 64 per wavefront: the small capacity overflows
    assert_rows(rows_of(engine.run_state(st)), want, "staged")
    with engine.plan(ewma_emit_rows=64):
        assert_rows(rows_of(engine.run_state(st)), want, "staged, 64 rows")
    with engine.plan(ewma_emit="lane"):
        assert_rows(rows_of(engine.run_state(st)), want, "lane")
    st.close()


# ---- 6. ARIMA ----
def arima_batches():
    """the minute shape of the streaming ARIMA test, plus a key with three points and a constant key"""
    K = 82
    batches = minute_batches(30000, 80, 48, (2, 5, 20, 33))
    out = []
    for b, (bk, bt, bv) in enumerate(batches):
        lo = (0, 2, 5, 20, 33)[b]
        ek, et, ev = [], [], []
        if b == 3:                                            # key 80: three points in all
            ek += [80, 80, 80]; et += [lo, lo + 2, lo + 5]; ev += [5_000_000, 7_000_000, 6_000_000]
        if b >= 2:                                            # key 81: constant
            ek += [81, 81, 81]; et += [lo, lo + 1, lo + 2]; ev += [42_000_000] * 3
        out.append((np.concatenate([bk, np.array(ek, np.uint64)]), np.concatenate([bt, T_BASE + 60 * np.array(et, np.int64)]),
                    np.concatenate([bv, np.array(ev, np.uint64)])))
    return K, out


def test_arima(engine):
    K, batches = arima_batches()
    st = new_state(engine, K, SER | TIMES)
    for bk, bt, bv in batches:
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
    n = st.export()["n"]
    assert n[80] == 3 and n[81] == 9
    for what in ("all batches", "trimmed"):
        for emit_all, maxiter in ((False, 0), (True, 0), (True, 5)):
            got, want = check(engine, st, "ARIMA", emit_all, what=what, maxiter=maxiter)
            assert got.stats["keys_no_result"] == want.stats["keys_no_result"] >= 2
            assert got.stats["arima_fits"] == want.stats["arima_fits"] > 0
            assert not np.isin(got["key_id"], (80, 81)).any()                 # keys with no result emit nothing
        st.trim(keep_points=14)
    st.close()


# ---- 7. restart ----
def test_restart(engine):
    K = 70
    st = new_state(engine, K)
    for bk, bt, bv in minute_batches(30000, K, 50, (10, 20, 35)):
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
    st.trim(keep_points=17)
    snap = snapshot(st)
    st2 = new_state(engine, K)
    st2.load(snap["state"])
    st2.load_history(*snap["history"])
    st2.load_series(*snap["series"])
    st2.load_times(snap["times"])
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        a = engine.run_state(st, algo=algo, emit_all=True)
        b = engine.run_state(st2, algo=algo, emit_all=True)
        assert a.n_rows > 0
        assert_rows(rows_of(b), rows_of(a), algo)
    st.close()
    st2.close()


# ---- 8. rejections leave the state unchanged ----


def test_rejections(engine):
    K = 50
    batches = minute_batches(12000, K, 30, (15,))
    for flags in (0, HIST, SER, HIST | SER, SER | TIMES, ALL):
        st = new_state(engine, K, flags)
        for bk, bt, bv in batches:
            engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
        snap = snapshot(st)
        for algo in ("EWMA", "DBSCAN", "ARIMA", "DROP"):
            ok = algo != "DROP" and (flags & (SER | TIMES)) == (SER | TIMES) and (algo != "DBSCAN" or flags & HIST)
            if ok:
                assert engine.run_state(st, algo=algo, emit_all=True).n_rows > 0
            else:
                with pytest.raises(TadError) as ei:
                    engine.run_state(st, algo=algo)
                assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT, (flags, algo)
        if flags == ALL:
            assert raw_run_state(engine, st, algo=0) == _capi.TAD_OK
            for bad in (dict(start_time=T_BASE), dict(end_time=T_BASE + 600), dict(start_time=T_BASE, end_time=T_BASE + 600),
                        dict(flags=_capi.TAD_FLAG_KEY_U32), dict(flags=_capi.TAD_FLAG_TIME_U32), dict(ewma_alpha=1.5)):
                assert raw_run_state(engine, st, algo=0, **bad) == _capi.TAD_ERR_INVALID_ARGUMENT, bad
            stale = new_state(engine, K)                      # the series imported, its times not yet
            stale.load(snap["state"])
            stale.load_history(*snap["history"])
            stale.load_series(*snap["series"])
            with pytest.raises(TadError):
                engine.run_state(stale)
            stale.load_times(snap["times"])
            assert_rows(rows_of(engine.run_state(stale)), rows_of(engine.run_state(st)), "times imported")
            stale.close()
        assert_same(snapshot(st), snap, flags)
        st.close()
    st = new_state(engine, K)                                 # an empty state: no rows, no error
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        for emit_all in (False, True):
            r = engine.run_state(st, algo=algo, emit_all=emit_all)
            assert r.n_rows == 0 and r.stats["n_points"] == 0 and r.stats["n_keys"] == 0 and r.stats["t0"] == 0
    st.close()


# ---- 9. two threads on one state ----
def test_two_threads_on_one_state(engine):
    K = 200
    st = new_state(engine, K)
    for bk, bt, bv in minute_batches(40000, K, 60, (30,)):
        engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum")
    serial = {algo: rows_of(engine.run_state(st, algo=algo, emit_all=True)) for algo in ("EWMA", "DBSCAN")}
    snap = snapshot(st)
    errors = []

    def worker(algo):
        try:
            for i in range(20):
                assert_rows(rows_of(engine.run_state(st, algo=algo, emit_all=True, job_id="%s-%d" % (algo, i))), serial[algo], (algo, i))
        except Exception as exc:      # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(algo,)) for algo in ("EWMA", "DBSCAN")]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert engine.jobs_in_flight() == 0
    assert_same(snapshot(st), snap)
    st.close()
