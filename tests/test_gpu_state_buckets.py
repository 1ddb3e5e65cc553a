"""GPU: tad_run_state_buckets (include/tad.h) — a streaming state judged in time buckets.  The defining property: with W' the rows
tad_run_state_keys judges for the same window and mask and W'' = W' with flow_end_s floored to its bucket's start, the call returns exactly
the rows tad_run returns for W'' with value_op = bucket_op.  Two references for every case: (R1) the engine's own tad_run over W'' built on
the host from export_series / export_times, rows and counters; (R2) oracle.tad_oracle.run_job over W'' (EWMA, DBSCAN; ARIMA through
arima_oracle).  Floats are compared as uint64 bit patterns.  Every case asserts its edge from host-side numbers (tests/buckets_model.py:
run lengths from the exported times, the chunk of a run's first and last point) before the engine is asked, and that the state is
unchanged afterwards.  The helpers come from tests/test_gpu_state_keys.py."""
import ctypes as C

import numpy as np
import pytest

import buckets_model as M
from oracle import arima_oracle as ao
from oracle import tad_oracle as orc
from theia_amd import TadEngine, TadError, _capi
from theia_amd.engine import DeviceArray
from state_helpers import (ALL, COOP_MIN_T, COUNTERS, EDGE_RUNS, EDGE_S, EDGE_T0, HIST_CHUNK, I64, ROW_FIELDS, SER, TIMES, T_BASE, U64, assert_rows,
                           assert_same, in_window, key_values, new_state, rows_of, run_times, snapshot, wide_values, window)

pytestmark = pytest.mark.gpu

NO_CHANGE = _capi.TAD_NO_CHANGE
INV = _capi.TAD_ERR_INVALID_ARGUMENT


# ---- the references ----
def r1(engine, K, rows, algo, op, emit_all, **kw):
    """the engine's own tad_run over W''"""
    k, t, v = rows
    return engine.run(algo, k, t, v, K, agg_flow="svc" if op == "sum" else "", value_op=op, emit_all=emit_all, **kw)


def r2_rows(rows, algo, op, emit_all, maxiter=0, **kw):
    """the oracle's job over W'': the rows the engine must return"""
    k, t, v = rows
    if algo == "ARIMA" and maxiter:
        kw["arima_fn"] = lambda x, counters=None: ao.calculate_arima_exact(x, maxiter=maxiter, counters=counters)
    want = orc.run_job(algo, k, t, v, op=op, **kw)
    if not emit_all:
        return {f: want[f] for f in ROW_FIELDS}
    pk, pt, pv = want["points"]
    sel = np.ones(pk.size, bool)
    if algo == "ARIMA":                                       # keys with no result emit nothing
        sel = np.repeat(np.array([r is not None for r in want["arima_results"]], bool), np.diff(want["ptr"]))
    sig = np.repeat(want["sigma"], np.diff(want["ptr"]))
    return {"key_id": pk[sel], "flow_end_s": pt[sel], "throughput": orc.u64_to_f64(pv)[sel], "algo_calc": want["calc_all"][sel],
            "stddev": sig[sel], "anomaly": want["anomaly_all"][sel].astype(np.uint8)}


def check(engine, st, W, bucket_s, origin=0, op="sum", win=(0, 0, 0), keep=None, algos=("EWMA", "DBSCAN"), emits=(True, False), params=None,
          snap=None, what="", oracle=True, keep_arg=None, mixed=True):
    """run_state_buckets equals R1 (rows and counters) and R2 (rows); the stats are the contract's; the state is unchanged.
    -> {(algo, emit_all): result}"""
    K = st.num_keys
    k, t, v = W
    m = in_window(k, t, *win)
    if keep is not None:
        m &= np.asarray(keep)[k.astype(I64)] != 0
    rows = (k[m], M.bucket_start(t[m], bucket_s, origin), v[m])
    bk, bt, bv = M.fold(k[m], t[m], v[m], bucket_s, origin, op)
    snap = snap or snapshot(st)
    out = {}
    for algo in algos:
        kw = dict((params or {}).get(algo, {}))
        for emit_all in emits:
            tag = (what, bucket_s, origin, op, win, algo, emit_all)
            got = engine.run_state_buckets(st, bucket_s, origin, op, *win, key_keep=keep if keep_arg is None else keep_arg, algo=algo,
                                           emit_all=emit_all, **kw)
            assert_same(snapshot(st), snap, (tag, "state changed"))
            gs = got.stats
            assert gs["rows_in"] == gs["rows_used"] == int(m.sum()), (tag, gs["rows_in"], int(m.sum()))
            assert gs["n_points"] == bk.size, (tag, gs["n_points"], bk.size)
            assert (gs["stage0_path"], gs["stage0_attempts"], gs["step"], gs["n_buckets"]) == (0, 0, 0, 0)
            out[(algo, emit_all)] = got
            if bk.size == 0:
                assert got.n_rows == 0 and gs["n_keys"] == 0 and gs["t0"] == 0 and gs["n_anomalies"] == 0, tag
                assert gs["host_syncs"] == (3 if k.size else 2), (tag, gs["host_syncs"])
                continue
            assert gs["host_syncs"] == 4, (tag, gs["host_syncs"])             # as built (tad.h): the keys call's 3 plus the bucket total
            assert gs["t0"] == int(bt.min()) and gs["n_keys"] == np.unique(bk).size, (tag, gs["t0"], gs["n_keys"])
            want = r1(engine, K, rows, algo, op, emit_all, **kw)
            assert_rows(rows_of(got), rows_of(want), (tag, "R1"))
            ws = want.stats
            for f in COUNTERS + ("t0",):
                assert gs[f] == ws[f], (tag, f, gs[f], ws[f])
            # the point moments are merged from per-key partials in another order than tad_run's: equal up to rounding, held as
            # tests/test_gpu_state_keys.py holds them (m2: a sum of n positive terms merged pairwise, a few units of 2^-53 each)
            x = orc.u64_to_f64(bv)
            assert abs(gs["pts_mean"] - x.mean()) <= 1e-12 * abs(x.mean()), (tag, gs["pts_mean"], x.mean())
            m2_err = abs(gs["pts_m2"] - ws["pts_m2"]) / ws["pts_m2"] if ws["pts_m2"] else abs(gs["pts_m2"])
            assert m2_err <= max(bk.size, 64) * 2.0 ** -50, (tag, gs["pts_m2"], ws["pts_m2"])
            if emit_all and algo != "ARIMA":
                assert np.array_equal(got["key_id"], bk) and np.array_equal(got["flow_end_s"], bt), (tag, "the model's buckets")
                assert np.array_equal(np.asarray(got["throughput"]).view(U64), orc.u64_to_f64(bv).view(U64)), (tag, "the model's folds")
            if not emit_all and mixed:
                assert 0 < got.n_rows < bk.size, (tag, got.n_rows, bk.size)   # mixed verdicts: no comparison is vacuous
            if algo == "ARIMA":
                assert gs["arima_fits"] > 0 and gs["arima_fits"] == ws["arima_fits"], (tag, gs["arima_fits"], ws["arima_fits"])
            if oracle:
                assert_rows(rows_of(got), r2_rows(rows, algo, op, emit_all, **kw), (tag, "R2"))
    return out


# ---- the states ----
def state_of(engine, K, k, t, v, seed=1, history=True):
    """a state of K keys fed the points (k, t, v), one row each, in a seeded order -> (state, W)"""
    k, t, v = np.asarray(k).astype(U64), np.asarray(t, I64), np.asarray(v).astype(U64)
    o = np.random.default_rng(seed).permutation(k.size)
    st = new_state(engine, K, ALL if history else SER | TIMES)
    if k.size:
        engine.run_stream(st, np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o]), value_op="max")
    return st, (window(st) if k.size else (np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64)))


def assert_runs(W, key, bucket_s, origin, runs):
    """host side: key's run lengths are `runs`; -> [(chunk of the run's first point, chunk of its last)] inside the key's segment"""
    k, t, _ = W
    tk = t[k == key]
    first, lens = M.run_lengths(np.full(tk.size, key, U64), tk, bucket_s, origin)
    assert list(lens) == list(runs), (key, list(lens), list(runs))
    return [(int(f) // HIST_CHUNK, int(f + n - 1) // HIST_CHUNK) for f, n in zip(first, lens)]


@pytest.fixture(scope="module")
def edge_state(engine):
    """EDGE_RUNS at EDGE_S-second buckets; values of 50 .. 62 bits, a third of them >= 2^63: sums wrap where the pieces of a run meet, and
    maxima lie on both sides of 2^63"""
    rng = np.random.default_rng(11)
    ks, ts, vs = [], [], []
    for key, runs in enumerate(EDGE_RUNS):
        tk = run_times(runs, EDGE_S, EDGE_T0, skip=(2,))
        ks.append(np.full(tk.size, key, I64)), ts.append(tk), vs.append(wide_values(tk.size, rng, top=0.33))
    st, W = state_of(engine, len(EDGE_RUNS), np.concatenate(ks), np.concatenate(ts), np.concatenate(vs))
    yield st, W, snapshot(st)
    st.close()


@pytest.mark.parametrize("op", ["sum", "max"])
def test_run_edges_inside_a_slice_a_chunk_and_over_several_chunks(engine, edge_state, op):
    st, W, snap = edge_state
    chunks = {key: assert_runs(W, key, EDGE_S, 0, runs) for key, runs in enumerate(EDGE_RUNS)}
    assert chunks[2][1] == (0, 0) and chunks[2][2] == (1, 1)            # ends on the chunk's last point; the next run opens a chunk
    assert chunks[1][2] == (0, 1) and chunks[3][1] == (0, 1) and chunks[4][1] == (0, 1)
    assert chunks[5] == [(0, 0), (1, 1), (2, 2)]
    assert chunks[6][1] == (0, 2) and chunks[7][1] == (0, 3) and chunks[9][0] == (0, 2)
    k, t, v = W
    if op == "sum":                                                     # the sum of the four-chunk run wraps, and more than once on the way
        run = v[k == 7][2047:2047 + 6145]
        assert int(run.astype(object).sum()) >> 64 >= 2
    else:
        assert (v >= U64(1 << 63)).any() and (v < U64(1 << 63)).any()
        bv = M.fold(k, t, v, EDGE_S, 0, "max")[2]
        assert (bv >= U64(1 << 63)).any() and (bv < U64(1 << 63)).any()
    check(engine, st, W, EDGE_S, 0, op, snap=snap, what="edges", mixed=False)


def test_the_edge_state_at_other_bucket_lengths_and_origins(engine, edge_state):
    st, W, snap = edge_state
    k, t, _ = W
    span = int(t.max() - t.min()) + 1
    assert 0 < int(t.min()) and int(t.max()) < (1 << 40) and span < (1 << 40)
    for bucket_s, origin in ((60, 0), (60, 1), (60, 59), (3600, 0), (3600, 3599), (1 << 40, 0)):   # (2^40: the largest documented bucket)
        first, lens = M.run_lengths(k, t, bucket_s, origin)
        if bucket_s == 60:
            assert lens.max() == 60 and lens.min() == 1                 # whole minutes and the partial ones at either end of a run of seconds
        if bucket_s > span:
            assert first.size == np.unique(k).size                      # one bucket per key
        check(engine, st, W, bucket_s, origin, "sum", emits=(True,), algos=("EWMA",), snap=snap, what="lengths", oracle=bucket_s != 60)


# ---- identity ----
@pytest.fixture(scope="module")
def small_state(engine):
    """14 keys of 0 .. 90 points at seeded seconds of 40 minutes"""
    lens = [30, 0, 1, 2, 64, 65, 90, 45, 0, 33, 63, 17, 80, 50]
    rng = np.random.default_rng(5)
    ks, ts, vs = [], [], []
    for key, n in enumerate(lens):
        off = np.sort(rng.choice(2400, size=n, replace=False))
        ks.append(np.full(n, key, I64)), ts.append(T_BASE + off.astype(I64)), vs.append(key_values(n, key, rng))
    st, W = state_of(engine, len(lens), np.concatenate(ks), np.concatenate(ts), np.concatenate(vs))
    yield st, W, snapshot(st), lens
    st.close()


@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN", "ARIMA"])
def test_a_bucket_of_one_second_is_the_keys_call(engine, small_state, algo):
    st, W, snap, lens = small_state
    kw = {"maxiter": 3} if algo == "ARIMA" else {}
    for emit_all in (True, False):
        want = engine.run_state_keys(st, None, algo=algo, emit_all=emit_all, **kw)
        got = engine.run_state_buckets(st, 1, algo=algo, emit_all=emit_all, **kw)
        assert_rows(rows_of(got), rows_of(want), (algo, emit_all))
        assert got.n_rows > 0
        for f in COUNTERS + ("t0", "rows_in", "rows_used"):
            assert got.stats[f] == want.stats[f], (algo, f)
        assert_same(snapshot(st), snap, "state changed")


def test_arima_and_parameters_away_from_their_defaults(engine, small_state):
    st, W, snap, lens = small_state
    check(engine, st, W, 60, 0, "sum", algos=("ARIMA",), params={"ARIMA": {"maxiter": 3}}, snap=snap, what="arima")
    check(engine, st, W, 120, 7, "max", algos=("EWMA", "DBSCAN"), emits=(False,), snap=snap, what="parameters", mixed=False,
          params={"EWMA": {"alpha": 0.25}, "DBSCAN": {"eps": 4.0e8, "min_samples": 3}})
    check(engine, st, W, 120, 7, "sum", algos=("ARIMA",), emits=(False,), params={"ARIMA": {"maxiter": 2}}, snap=snap, what="maxiter", mixed=False)


# ---- key shapes ----
@pytest.fixture(scope="module")
def shape_state(engine):
    """257 keys: 0, 1, 2, 2047, 2048, 2049 and 4097 points and short ones, empty keys between full ones, at seeded seconds of three hours"""
    K = 257
    lens = [(5 * j + 1) % 23 for j in range(K)]
    for key, n in ((0, 0), (1, 1), (2, 2), (3, 2047), (4, 0), (5, 2048), (6, 2049), (7, 0), (8, 0), (9, 4097), (255, 0), (256, 1)):
        lens[key] = n
    rng = np.random.default_rng(8)
    ks, ts, vs = [], [], []
    for key, n in enumerate(lens):
        off = np.sort(rng.choice(10800, size=n, replace=False))
        if key == 20:                                         # every point in a bucket of its own at 60 s, on the bucket starts
            off = 60 * np.arange(n)
        if key == 21:                                         # all points in one minute
            off = 600 + np.arange(n)
        ks.append(np.full(n, key, I64)), ts.append((T_BASE // 60) * 60 + off.astype(I64)), vs.append(key_values(n, key, rng))
    st, W = state_of(engine, K, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs))
    assert np.array_equal(st.export_series()[0], np.asarray(lens).astype(U64))
    yield st, W, snapshot(st), lens
    st.close()


def test_key_shapes_in_one_state(engine, shape_state):
    st, W, snap, lens = shape_state
    k, t, v = W
    first, rl = M.run_lengths(k, t, 60)
    assert lens[20] > 1 and (rl[k[first] == 20] == 1).all() and (rl[k[first] == 21] == lens[21]).all() and lens[21] > 1
    assert rl[k[first] == 9].max() > 1
    nb = np.bincount(M.fold(k, t, v, 60)[0].astype(I64), minlength=st.num_keys)
    assert nb.max() < COOP_MIN_T                                        # EWMA: every bucketed key stays on a lane
    check(engine, st, W, 60, 0, "sum", snap=snap, what="shapes")
    check(engine, st, W, 3600, 1800, "max", snap=snap, what="shapes, hours", emits=(True,))


@pytest.mark.parametrize("K", [1, 64, 65])
def test_key_counts_around_a_wavefront_of_keys(engine, K):
    rng = np.random.default_rng(K)
    n = 75
    ks = np.repeat(np.arange(K), n)
    ts = np.concatenate([T_BASE + np.sort(rng.choice(1500, size=n, replace=False)) for _ in range(K)])
    st, W = state_of(engine, K, ks, ts, np.concatenate([key_values(n, key, rng) for key in range(K)]))
    try:
        check(engine, st, W, 60, 0, "sum", what="K=%d" % K)
    finally:
        st.close()


def test_one_key_of_100000_points_among_300_short_ones(engine):
    rng = np.random.default_rng(3)
    K, long_key, n_long = 301, 150, 100_000
    lens = [int(x) for x in rng.integers(1, 60, size=K)]
    lens[long_key] = n_long
    ks, ts, vs = [], [], []
    for key, n in enumerate(lens):
        off = np.arange(n) if key == long_key else np.sort(rng.choice(n_long, size=n, replace=False))
        ks.append(np.full(n, key, I64)), ts.append(T_BASE + off.astype(I64)), vs.append(key_values(n, key, rng))
    st, W = state_of(engine, K, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs))
    try:
        assert (n_long + HIST_CHUNK - 1) // HIST_CHUNK == 49                 # the long key spreads over 49 chunks
        # EWMA's other route: the long key has >= 512 buckets and few keys share the state — a wavefront of its own; the rest stay on lanes
        nb = np.bincount(M.fold(*W, 60)[0].astype(I64), minlength=K)
        assert nb[long_key] >= COOP_MIN_T > np.delete(nb, long_key).max()
        check(engine, st, W, 60, 0, "sum", what="long key", emits=(False,))
    finally:
        st.close()


# ---- time arithmetic ----
def test_times_below_zero_on_a_bucket_start_and_one_second_before(engine):
    """keys around time 0 and around bucket starts: a point exactly on a start opens a bucket, the second before closes one"""
    rng = np.random.default_rng(4)
    K, ks, ts, vs = 6, [], [], []
    for key in range(K):
        off = np.unique(np.concatenate([np.array([-3600, -3541, -3540, -61, -60, -1, 0, 1, 59, 60, 61, 119, 120, 3599, 3600]),
                                        rng.integers(-7200, 7200, size=50)]))
        ks.append(np.full(off.size, key, I64)), ts.append(off.astype(I64)), vs.append(key_values(off.size, key, rng))
    st, W = state_of(engine, K, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs))
    try:
        k, t, _ = W
        assert (t < 0).any() and (t == -1).any() and (t == 0).any()
        b = M.bucket_start(t, 60)
        assert b[t == -1][0] == -60 and b[t == -60][0] == -60 and b[t == -61][0] == -120 and b[t == 59][0] == 0 and b[t == 60][0] == 60
        assert M.bucket_start(np.array([-1, 0, 1]), 60, 1).tolist() == [-59, -59, 1]
        for bucket_s, origin in ((60, 0), (60, 1), (60, 59), (3600, 0), (1, 0), (1 << 20, 0)):
            check(engine, st, W, bucket_s, origin, "sum", algos=("EWMA",), emits=(True,), what="below zero")
        check(engine, st, W, 60, 59, "max", what="below zero, detectors")
    finally:
        st.close()


# ---- window, then bucket ----
def test_the_window_is_applied_to_the_raw_points_first(engine, shape_state):
    st, W, snap, lens = shape_state
    k, t, v = W
    base = (T_BASE // 60) * 60
    # from_t / to_t inside a bucket: the partial buckets at either end hold only the window's points
    win = (base + 3600 + 17, base + 7200 + 43, 0)
    m = in_window(k, t, *win)
    bt = M.fold(k[m], t[m], v[m], 60)[1]
    assert bt.min() == base + 3600 and bt.max() == base + 7200 and t[m].min() >= win[0] and t[m].max() < win[1]
    check(engine, st, W, 60, 0, "sum", win=win, snap=snap, what="bounds inside a bucket")
    # keep_points cuts a bucket: key 21 holds one minute of points
    win = (0, 0, 5)
    assert lens[21] > 5 and M.fold(k[in_window(k, t, *win)], t[in_window(k, t, *win)], v[in_window(k, t, *win)], 60)[0].size < in_window(k, t, *win).sum()
    check(engine, st, W, 60, 0, "sum", win=win, snap=snap, what="keep_points", mixed=False)
    # a mask, from the host and from the device
    keep = (np.arange(st.num_keys) % 3 != 1).astype(np.uint8)
    assert keep[9] and keep[3] and not keep[1]
    check(engine, st, W, 60, 0, "max", keep=keep, snap=snap, what="mask", emits=(False,))
    dev = DeviceArray.from_host(engine, np.concatenate([keep, np.zeros(-keep.size % 8, np.uint8)]).view(U64))
    check(engine, st, W, 60, 0, "sum", win=(base + 600, 0, 0), keep=keep, keep_arg=dev, snap=snap, what="device mask", algos=("EWMA",), emits=(True,))
    # a window that leaves every key whole (P == S) still buckets; so does no window at all (above)
    win = (int(t.min()), int(t.max()) + 1, 0)
    assert in_window(k, t, *win).all()
    res = check(engine, st, W, 60, 0, "sum", win=win, snap=snap, what="P == S", algos=("EWMA",), emits=(True,))
    assert res[("EWMA", True)].n_rows < k.size
    # an empty window
    check(engine, st, W, 60, 0, "sum", win=(int(t.max()) + 10, 0, 0), snap=snap, what="empty window")


def test_an_empty_state_gives_no_rows(engine):
    st, W = state_of(engine, 5, [], [], [])
    try:
        check(engine, st, W, 60, what="empty state")
    finally:
        st.close()


def test_dbscan_on_both_sides_of_the_history_rule_of_the_raw_window(engine, shape_state):
    st, W, snap, lens = shape_state
    k, t, v = W
    S = k.size
    lib = engine._lib
    base = (T_BASE // 60) * 60
    small, large = (base + 9000, 0, 0), (base + 1200, 0, 0)
    assert lib.tad_window_history_by_sort(int(in_window(k, t, *small).sum()), S) == 1
    assert lib.tad_window_history_by_sort(int(in_window(k, t, *large).sum()), S) == 0      # the keys call would subtract: the buckets never do
    for win in (small, large):
        check(engine, st, W, 60, 0, "sum", win=win, algos=("DBSCAN",), snap=snap, what="history rule")


# ---- since ----
def check_since(engine, st, W, bucket_s, origin=0, op="sum", since_t=0, key_since=None, keep=None, win=(0, 0, 0), algos=("EWMA", "DBSCAN"),
                emits=(True, False), snap=None, what="", since_arg=None, params=None):
    """the call with a since against the same call without one (effective mask), filtered on the host by the model's rule"""
    K = st.num_keys
    eff = np.ones(K, np.uint8) if keep is None else (np.asarray(keep) != 0).astype(np.uint8)
    if key_since is not None:
        eff &= (np.asarray(key_since, I64) != NO_CHANGE).astype(np.uint8)
    snap = snap or snapshot(st)
    out = {}
    for algo in algos:
        kw = dict((params or {}).get(algo, {}))
        for emit_all in emits:
            tag = (what, bucket_s, origin, since_t, algo, emit_all)
            full_res = engine.run_state_buckets(st, bucket_s, origin, op, *win, key_keep=eff, algo=algo, emit_all=emit_all, **kw)
            full = rows_of(full_res)
            sel = M.reported(full["key_id"], full["flow_end_s"], bucket_s, origin, since_t, key_since)
            got = engine.run_state_buckets(st, bucket_s, origin, op, *win, key_keep=keep, key_since=key_since if since_arg is None else since_arg,
                                           since_t=since_t, algo=algo, emit_all=emit_all, **kw)
            assert_same(snapshot(st), snap, (tag, "state changed"))
            assert_rows(rows_of(got), {f: a[sel] for f, a in full.items()}, (tag, "the same call without a since, filtered"))
            for f in ("rows_in", "rows_used", "n_points", "n_keys", "t0"):
                assert got.stats[f] == full_res.stats[f], (tag, f)
            out[(algo, emit_all)] = (got, int(sel.sum()), sel.size)
    return out


def test_since_on_a_bucket_start_inside_a_bucket_before_and_after_everything(engine, shape_state):
    st, W, snap, lens = shape_state
    k, t, v = W
    base = (T_BASE // 60) * 60
    on = check_since(engine, st, W, 60, since_t=base + 5400, snap=snap, what="on a start")
    # inside a bucket: the bucket that holds the threshold is reported whole — the same rows as from its start
    inside = check_since(engine, st, W, 60, since_t=base + 5400 + 31, snap=snap, what="inside")
    for key in on:
        assert on[key][1] == inside[key][1] and 0 < on[key][1] < on[key][2], key
        assert_rows(rows_of(on[key][0]), rows_of(inside[key][0]), key)
    before = check_since(engine, st, W, 60, since_t=int(t.min()) - 1000, snap=snap, what="before everything", emits=(True,))
    assert all(n == total for _, n, total in before.values())
    after = check_since(engine, st, W, 60, since_t=int(t.max()) + 1000, snap=snap, what="after everything")
    assert all(r.n_rows == 0 for r, _, _ in after.values())
    check_since(engine, st, W, 3600, 1800, "max", since_t=base + 4000, win=(base + 700, 0, 0), snap=snap, what="origin and window", algos=("DBSCAN",))


def test_key_since_with_no_change_from_both_memories(engine, shape_state):
    st, W, snap, lens = shape_state
    K = st.num_keys
    base = (T_BASE // 60) * 60
    ks = np.full(K, NO_CHANGE, I64)
    ks[[3, 5, 6, 9, 20, 21, 30, 31, 256]] = [base + 3000, base + 29, base + 10799, base + 7000, base + 61, base + 630, base, base + 10 ** 6, 5]
    keep = np.ones(K, np.uint8)
    keep[6] = 0
    res = check_since(engine, st, W, 60, key_since=ks, keep=keep, since_t=base + 100, snap=snap, what="host")
    assert all(0 < n < total for _, n, total in res.values())
    dev = DeviceArray.from_host(engine, ks)
    check_since(engine, st, W, 60, key_since=ks, since_arg=dev, snap=snap, what="device", emits=(False,))
    check_since(engine, st, W, 60, key_since=ks, algos=("ARIMA",), emits=(True,), keep=(np.arange(K) > 200).astype(np.uint8), snap=snap,
                what="arima", params={"ARIMA": {"maxiter": 2}})


def test_a_report_taken_as_it_stands_from_replace_stream_changes(engine):
    rng = np.random.default_rng(6)
    K, n = 40, 120
    base = (T_BASE // 60) * 60
    ks = np.repeat(np.arange(K), n)
    ts = np.concatenate([base + np.sort(rng.choice(3000, size=n, replace=False)) for _ in range(K)])
    st, W = state_of(engine, K, ks, ts, np.concatenate([key_values(n, key, rng) for key in range(K)]))
    try:
        # a re-read of ten minutes: some keys get other values at held seconds, some a new second, most nothing
        k, t, v = W
        m = (t >= base + 1800) & (t < base + 2400) & (k % U64(4) == 0)
        nk, nt, nv = k[m], t[m].copy(), v[m] + U64(12345)
        nk, nt, nv = np.append(nk, U64(7)), np.append(nt, base + 2000 + 3600), np.append(nv, U64(4_000_000_000))
        rep = engine.replace_stream_changes(st, nk, nt, nv, changes="device", value_op="max")
        since = rep["key_since"]
        host = np.asarray(since.to_host(), I64)[:K]
        assert 0 < int((host != NO_CHANGE).sum()) < K and rep["keys_changed"] == int((host != NO_CHANGE).sum())
        assert (host[host != NO_CHANGE] % 60 != 0).any()                                 # a first changed second inside a minute
        res = check_since(engine, st, window(st), 60, key_since=host, since_arg=since, what="report")
        assert all(0 < n_ < total for _, n_, total in res.values())
    finally:
        st.close()


# ---- atomicity and refusals ----
def test_a_workspace_limit_too_small_for_the_view_fails_with_the_state_unchanged():
    small = TadEngine(device=0, workspace_limit=1 << 20)
    try:
        K, n = 700, 200                                        # 140 000 points: a view of 16 B per bucket needs more than 1 MiB at one second
        st = new_state(small, K, SER | TIMES)
        rng = np.random.default_rng(2)
        for b in range(10):                                    # small batches: the feed itself stays under the limit
            k = np.repeat(np.arange(K, dtype=U64), n // 10)
            t = T_BASE + b * 100 + np.tile(np.arange(n // 10, dtype=I64), K)
            small.run_stream(st, k, t, rng.integers(1, 1 << 30, size=k.size).astype(U64), value_op="max")
        snap = snapshot(st)
        assert st.series_points() * 16 > (1 << 20)
        with pytest.raises(TadError) as ei:
            small.run_state_buckets(st, 1)
        assert ei.value.code == _capi.TAD_ERR_GRID_TOO_LARGE
        assert_same(snapshot(st), snap, "state changed")
        got = small.run_state_buckets(st, 3600, emit_all=True)                           # few buckets: the same state fits
        assert got.n_rows == got.stats["n_points"] <= 2 * K and got.stats["rows_in"] == K * n
        assert_same(snapshot(st), snap, "state changed")
        st.close()
    finally:
        small.close()


def test_refusals(engine, small_state):
    st, W, snap, lens = small_state
    lib, K = engine._lib, st.num_keys
    BW = _capi.BucketWindow
    res = C.POINTER(_capi.Result)()
    job = _capi.Job(algo=_capi.TAD_ALGO["EWMA"])

    def call(w, j=job, state=st):
        return lib.tad_run_state_buckets(engine._h, state._h, C.byref(j), C.byref(w) if w is not None else None, 0, C.byref(res))

    def ok(**kw):
        d = dict(bucket_s=60, bucket_origin=0, bucket_op=_capi.TAD_OP["sum"])
        d.update(kw)
        return BW(**d)
    assert call(None) == INV
    for bad in (ok(bucket_s=0), ok(bucket_s=-60), ok(bucket_origin=-1), ok(bucket_origin=60), ok(bucket_origin=61), ok(bucket_s=1, bucket_origin=1),
                ok(bucket_op=_capi.TAD_OP["auto"]), ok(bucket_op=7), ok(from_t=10, to_t=5), ok(key_memory=5, key_keep=1, num_keys=K)):
        assert call(bad) == INV
    assert call(ok(), _capi.Job(algo=_capi.TAD_ALGO["DROP"])) == INV
    assert b"DROP" in lib.tad_last_error(engine._h)
    assert call(ok(), _capi.Job(algo=_capi.TAD_ALGO["EWMA"], start_time=5)) == INV
    assert call(ok(), _capi.Job(algo=_capi.TAD_ALGO["EWMA"], ewma_alpha=1.5)) == INV
    assert call(ok(), _capi.Job(algo=_capi.TAD_ALGO["EWMA"], flags=_capi.TAD_FLAG_KEY_U32)) == INV
    plain = engine.state_create(K)
    assert call(ok(), state=plain) == INV
    plain.close()
    nohist = new_state(engine, K, SER | TIMES)
    assert call(ok(), _capi.Job(algo=_capi.TAD_ALGO["DBSCAN"]), state=nohist) == INV
    nohist.close()
    with pytest.raises(TadError):
        engine.run_state_buckets(st, 60, key_since=np.zeros(K - 1, I64))
    with pytest.raises(TadError):
        engine.run_state_buckets(st, 60, op="auto")
    mis = np.zeros(K + 1, I64)
    assert call(ok(key_since=mis.ctypes.data + 4, num_keys=K)) == INV
    assert call(ok(key_since=mis.ctypes.data, num_keys=K + 1)) == INV
    assert lib.tad_run_state_buckets(None, st._h, C.byref(job), C.byref(ok()), 0, C.byref(res)) == INV
    assert call(ok()) == 0
    lib.tad_result_free(engine._h, res)
    assert_same(snapshot(st), snap, "state changed")
