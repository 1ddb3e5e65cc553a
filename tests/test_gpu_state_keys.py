"""GPU: the window calls over selected keys of a streaming state (tad_run_state_keys / tad_drop_state_keys, include/tad.h).  The defining
property: with W' the window's rows of tad_run_state_window / tad_drop_state and W'' the rows of W' whose key has key_keep[key] != 0, the
call returns exactly the rows tad_run returns for W''.  Two references for every case: (R1) the rows of the window call itself, filtered
on the host by the mask; (R2) the engine's own tad_run over W'' built from export_series / export_times, which also gives the counters.
EWMA and DBSCAN have a third, oracle.tad_oracle.run_job on W'' (DROP: oracle.drop_oracle).  Floats are compared as uint64 bit patterns;
every case asserts its edge from host-side numbers first and that the state is unchanged afterwards.  The helpers follow
tests/test_gpu_state_window.py (copied, not imported)."""
import ctypes as C

import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadError, _capi
from theia_amd.engine import DeviceArray
from state_helpers import (COOP_MIN_T, COUNTERS, HIST_CHUNK, SER, TIMES, T_BASE, U64, assert_rows, assert_same, drop_oracle_rows, in_window,
                           make_state, new_state, order_sensitive, rows_of, snapshot, window, window_oracle_rows)

pytestmark = pytest.mark.gpu


# ---- the states: key k holds lens[k] points at seconds starts[k] + 0, 1, 2 ... (or at seeded seconds), values around a per-key base ----


def check_keys(engine, st, W, keep, win=(0, 0, 0), algos=("EWMA", "DBSCAN"), what="", params=None, snap=None, key_arg=None, emits=(True, False)):
    """run_state_keys equals R1 (the window call's rows, filtered), R2 (tad_run over W'': rows and counters) and, for EWMA and DBSCAN,
    the oracle on W''; the state is unchanged.  -> {(algo, emit_all): result}"""
    K = st.num_keys
    keep = np.asarray(keep).astype(np.uint8)
    assert keep.size == K
    m = in_window(W[0], W[1], *win) & (keep[W[0].astype(np.int64)] != 0)
    P2 = int(m.sum())
    snap = snap or snapshot(st)
    out = {}
    for algo in algos:
        kw = dict((params or {}).get(algo, {}))
        for emit_all in emits:
            tag = (what, win, algo, emit_all)
            got = engine.run_state_keys(st, keep if key_arg is None else key_arg, *win, algo=algo, emit_all=emit_all, **kw)
            assert_same(snapshot(st), snap, (tag, "state changed"))
            gs = got.stats
            print("%s: selected %d of %d keys, %d of %d points, rows %d" % (tag, int((keep != 0).sum()), K, P2, W[0].size, got.n_rows))
            assert gs["rows_in"] == gs["rows_used"] == gs["n_points"] == P2, (tag, gs["n_points"], P2)
            assert (gs["stage0_path"], gs["stage0_attempts"], gs["step"], gs["n_buckets"]) == (0, 0, 0, 0)
            full = rows_of(engine.run_state_window(st, *win, algo=algo, emit_all=emit_all, **kw))
            sel = keep[full["key_id"].astype(np.int64)] != 0
            assert_rows(rows_of(got), {f: a[sel] for f, a in full.items()}, (tag, "R1"))
            out[(algo, emit_all)] = got
            if P2 == 0:
                assert got.n_rows == 0 and gs["n_keys"] == 0 and gs["t0"] == 0 and gs["n_anomalies"] == 0, tag
                continue
            ref = engine.run(algo, W[0][m], W[1][m], W[2][m], K, agg_flow="svc", value_op="sum", emit_all=emit_all, **kw)
            assert_rows(rows_of(got), rows_of(ref), (tag, "R2"))
            for f in COUNTERS + ("t0",):
                assert gs[f] == ref.stats[f], (tag, f, gs[f], ref.stats[f])
            assert gs["n_keys"] == np.unique(W[0][m]).size and gs["t0"] == int(W[1][m].min()), tag
            # the point moments are merged from per-key partials in another order than tad_run's: equal up to rounding (tad.h).  The mean
            # as tests/test_gpu_state_run.py holds it; m2, a sum of n positive terms merged pairwise, to n * 2^-50 (a few units of 2^-53 each)
            x = orc.u64_to_f64(W[2][m])
            assert abs(gs["pts_mean"] - x.mean()) <= 1e-12 * abs(x.mean()), (tag, gs["pts_mean"], x.mean())
            m2_err = abs(gs["pts_m2"] - ref.stats["pts_m2"]) / ref.stats["pts_m2"] if ref.stats["pts_m2"] else abs(gs["pts_m2"])
            print("%s: pts_m2 relative difference %.3g, bound %.3g" % (tag, m2_err, max(P2, 64) * 2.0 ** -50))
            assert m2_err <= max(P2, 64) * 2.0 ** -50, (tag, gs["pts_m2"], ref.stats["pts_m2"])
            if emit_all:
                assert got.n_rows == P2 or algo == "ARIMA", tag
            if algo != "ARIMA":
                assert_rows(rows_of(got), window_oracle_rows(W, m, algo, emit_all, **kw), (tag, "oracle"))
    return out


# ---- 1. key counts and masks ----
MASKS = ("all", "none", "key 0 only", "key K - 1 only", "every second key", "every 64th key", "keys 256 .. K - 1", "a random half")


def mask_of(name, K, seed=0):
    k = np.arange(K)
    return {"all": np.ones(K, bool), "none": np.zeros(K, bool), "key 0 only": k == 0, "key K - 1 only": k == K - 1, "every second key": k % 2 == 0,
            "every 64th key": k % 64 == 0, "keys 256 .. K - 1": k >= 256,
            "a random half": np.random.default_rng(K + seed).random(K) < 0.5}[name].astype(np.uint8)


@pytest.fixture(scope="module")
def count_states(engine):
    """one state per key count, series of 1 .. 40 points at seeded seconds of an hour: built once, read by every mask's case"""
    made = {}
    for K in (1, 255, 256, 257, 1025):
        lens = 1 + (np.arange(K) * 7 + 3) % 40
        if K == 1:
            lens = np.array([40])
        st, W = make_state(engine, lens, seed=K, spread=3600)
        made[K] = (st, W, snapshot(st), lens)
    yield made
    for st, _, _, _ in made.values():
        st.close()


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("K", (1, 255, 256, 257, 1025))
def test_key_counts_and_masks(engine, count_states, K, name):
    st, W, snap, lens = count_states[K]
    keep = mask_of(name, K)
    assert set(lens.tolist()) == (set(range(1, 41)) if K > 1 else {40})
    lo, hi = int(W[1].min()), int(W[1].max())
    wins = [(0, 0, 0), (lo + 600, hi - 600, 0), (0, 0, 5)]
    for win in wins:
        got = check_keys(engine, st, W, keep, win, what=(K, name), snap=snap)
        if name == "all":                                     # the whole selection is the window call (and, unwindowed, run_state)
            assert got[("EWMA", True)].stats["host_syncs"] == 3
        if name == "none" or (name == "keys 256 .. K - 1" and K <= 256):
            assert not keep.any() and got[("EWMA", True)].n_rows == 0 and got[("EWMA", True)].stats["host_syncs"] == 3


# ---- 2. degenerate keys ----
def test_selected_keys_without_points_outside_the_window_and_cut_by_count(engine):
    lens = np.array([0, 12, 0, 30, 9, 0, 30, 30, 1, 0])
    starts = [0, 0, 0, 0, 5000, 0, 0, 40, 0, 0]              # key 4 lies wholly after the others; key 7 starts later
    st, W = make_state(engine, lens, seed=3, starts=starts)
    K = lens.size
    snap = snapshot(st)
    # selected keys that hold no point (0, 2, 9) beside ones that do, and with nothing else selected
    for sel in ((0, 1, 2, 9), (0, 2, 5, 9), (3,), (0,)):
        keep = np.isin(np.arange(K), sel).astype(np.uint8)
        assert (lens[list(sel)] == 0).any() or len(sel) == 1
        check_keys(engine, st, W, keep, what=("no point", sel), snap=snap)
    # selected keys wholly outside [from_t, to_t): key 4 (after), key 1 (before from_t = 20), beside keys the window cuts
    win = (T_BASE + 20, T_BASE + 60, 0)
    mw = in_window(W[0], W[1], *win)
    n_in = np.bincount(W[0][mw].astype(np.int64), minlength=K)
    assert n_in[4] == 0 and n_in[1] == 0 and 0 < n_in[3] < lens[3] and 0 < n_in[7] < lens[7]
    for sel in ((1, 4), (1, 3, 4), (4, 7), (3, 6, 7)):
        check_keys(engine, st, W, np.isin(np.arange(K), sel).astype(np.uint8), win, what=("outside", sel), snap=snap)
    # keep_points cutting selected keys only: the keys of 30 points selected, the ones a count of 10 leaves whole not
    keep = (lens > 12).astype(np.uint8)
    assert keep.sum() == 3 and (lens[keep == 0] <= 12).all()
    check_keys(engine, st, W, keep, (0, 0, 10), what="count cuts the selected keys", snap=snap)
    check_keys(engine, st, W, 1 - keep, (0, 0, 12), what="count cuts no selected key", snap=snap)
    st.close()


# ---- 3. the copy's chunks: long and short neighbours, selected and not ----
CHUNK_LENS = (2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def chunk_state(engine):
    """keys 0, 2, 4, 6 hold 2047, 2048, 2049 and 4097 points, a neighbour of 5 points behind each: the first key of the state is long,
    the last one short; a second state holds them the other way round"""
    made = {}
    for name, lens in (("long first", [2047, 5, 2048, 5, 2049, 5, 4097, 5]), ("short first", [5, 2047, 5, 2048, 5, 2049, 5, 4097])):
        st, W = make_state(engine, np.array(lens), seed=len(name))
        made[name] = (st, W, snapshot(st), np.array(lens))
    yield made
    for st, _, _, _ in made.values():
        st.close()


@pytest.mark.parametrize("selected", ("long", "short"))
@pytest.mark.parametrize("layout", ("long first", "short first"))
def test_long_and_short_neighbours_at_every_chunk_edge(engine, chunk_state, layout, selected):
    st, W, snap, lens = chunk_state[layout]
    K = lens.size
    keep = ((lens > 5) == (selected == "long")).astype(np.uint8)
    chunks = np.where(lens > HIST_CHUNK, -(-lens // HIST_CHUNK), 1)
    assert sorted(lens[lens > 5].tolist()) == list(CHUNK_LENS) and sorted(chunks[lens > 5].tolist()) == [1, 1, 2, 3]
    assert keep[0] != keep[K - 1] and {int(keep[0]), int(keep[K - 1])} == {0, 1}      # the first and the last key: one selected, one not
    S = W[0].size
    P = int(lens[keep != 0].sum())
    assert engine._lib.tad_window_history_by_sort(P, S) == (1 if selected == "short" else 0)
    # unwindowed (every selected key whole), and a window that cuts the long keys at element 2047 / 2049 of their segments
    for win in ((0, 0, 0), (T_BASE + 2047, 0, 0), (0, T_BASE + 2049, 0), (0, 0, 2048)):
        check_keys(engine, st, W, keep, win, what=(layout, selected), snap=snap, params={"EWMA": {"alpha": 0.3}})


# ---- 4. routing ----
def test_a_selected_key_on_either_side_of_512_points_beside_unselected_long_keys(engine):
    lens = np.array([3000, 511, 3000, 512, 3000, 513, 9, 3000])
    st, W = make_state(engine, lens, seed=5)
    K = lens.size
    snap = snapshot(st)
    for sel in ((1,), (3,), (5,), (1, 3, 5, 6)):
        keep = np.isin(np.arange(K), sel).astype(np.uint8)
        assert (lens[keep == 0] >= COOP_MIN_T).sum() >= 4 and K <= 8192      # the view's routing: 512 points, whatever was left out
        got = check_keys(engine, st, W, keep, what=("coop", sel), snap=snap, params={"EWMA": {"alpha": 0.3}})
        assert got[("EWMA", False)].n_rows > 0
    st.close()


def test_an_all_zero_window_with_a_mask_is_not_the_whole_state(engine):
    lens = np.array([20, 30, 25, 40, 8])
    st, W = make_state(engine, lens, seed=6)
    keep = np.array([1, 0, 1, 0, 0], np.uint8)
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        got = check_keys(engine, st, W, keep, algos=(algo,), what="all-zero window")[(algo, True)]
        whole = engine.run_state_window(st, algo=algo, emit_all=True)
        assert got.stats["host_syncs"] == 3 and whole.stats["host_syncs"] == 2
        assert got.stats["n_points"] == 45 and whole.stats["n_points"] == 123 and (algo == "ARIMA" or (got.n_rows, whole.n_rows) == (45, 123))
    none = engine.run_state_keys(st, None, algo="EWMA", emit_all=True)       # no mask at all: the window call itself
    assert none.stats["host_syncs"] == 2 and none.n_rows == 123
    allk = engine.run_state_keys(st, np.ones(5, np.uint8), algo="EWMA", emit_all=True)   # every point selected: the state's own arrays
    assert allk.stats["host_syncs"] == 3 and allk.n_rows == 123
    st.close()


# ---- 5. DBSCAN on both history rules ----
def test_dbscan_sorts_the_selection_or_subtracts_the_rest(engine):
    # keys 0 .. 5; key 2 holds 2049 points that tie with its selected neighbours' values
    lens = np.array([700, 900, 2049, 800, 300, 60])
    st, W = make_state(engine, lens, seed=9, ties=(1, 2, 3))
    K, S = lens.size, int(lens.sum())
    snap = snapshot(st)
    hv = st.export_history()[1]
    off = np.concatenate([[0], np.cumsum(lens)])
    assert set(hv[off[1]:off[2]].tolist()) & set(hv[off[2]:off[3]].tolist()) & set(hv[off[3]:off[4]].tolist())   # values that tie across the keys
    cases = {"by sort": (4, 5), "by sort, the long key": (2,), "subtract, the long key between two selected ones": (0, 1, 3, 4, 5),
             "subtract, the long key selected": (1, 2, 3)}
    for name, sel in cases.items():
        keep = np.isin(np.arange(K), sel).astype(np.uint8)
        P = int(lens[list(sel)].sum())
        by_sort = 2 * P <= S
        assert by_sort == name.startswith("by sort"), (name, P, S)
        assert bool(engine._lib.tad_window_history_by_sort(P, S)) == by_sort
        check_keys(engine, st, W, keep, algos=("DBSCAN",), what=name, snap=snap, params={"DBSCAN": {"eps": float(1 << 22), "min_samples": 4}})
        check_keys(engine, st, W, keep, algos=("DBSCAN",), what=name, snap=snap)
    # with a window on top: the selected keys cut, P counted inside the window
    win = (T_BASE + 100, T_BASE + 2000, 0)
    for sel, by_sort in (((1, 3), True), ((0, 1, 2, 3), False)):
        keep = np.isin(np.arange(K), sel).astype(np.uint8)
        P = int((in_window(W[0], W[1], *win) & (keep[W[0].astype(np.int64)] != 0)).sum())
        assert 0 < P and (2 * P <= S) == by_sort and bool(engine._lib.tad_window_history_by_sort(P, S)) == by_sort, (sel, P, S)
        check_keys(engine, st, W, keep, win, algos=("DBSCAN",), what=("windowed", sel), snap=snap, params={"DBSCAN": {"eps": float(1 << 22), "min_samples": 4}})
    st.close()


# ---- 6. ARIMA: the counters show that a key that is not selected costs no fit ----
def test_arima_fits_follow_the_selection(engine):
    lens = 4 + (np.arange(24) * 5) % 37                       # 24 keys of 4 .. 40 points
    assert lens.min() == 4 and lens.max() == 40 and lens.size == 24
    st, W = make_state(engine, lens, seed=24, history=False)
    assert (W[2] > 0).all() and all(np.unique(W[2][W[0] == k]).size > 1 for k in range(24))     # positive, non-constant
    snap = snapshot(st)
    whole = engine.run_state_window(st, algo="ARIMA", emit_all=True)
    fits = {}
    for sel in ((17,), (2, 11, 23), tuple(range(24))):
        keep = np.isin(np.arange(24), sel).astype(np.uint8)
        got = check_keys(engine, st, W, keep, algos=("ARIMA",), what=("arima", len(sel)), snap=snap)[("ARIMA", True)]
        fits[len(sel)] = got.stats["arima_fits"]
        assert got.stats["n_keys"] == len(sel)
    assert 0 < fits[1] < fits[3] < fits[24] == whole.stats["arima_fits"], fits
    assert fits[1] < whole.stats["arima_fits"]
    st.close()


# ---- 7. DROP ----
DAY = 86400
D_BASE = 1660176000


def drop_values(rng, n):
    nb = rng.integers(50, 63, size=n)
    lo = np.left_shift(np.uint64(1), (nb - 1).astype(np.uint64))
    return lo + (rng.integers(0, 1 << 62, size=n, dtype=np.uint64) & (lo - np.uint64(1)))


def test_drop_state_keys_on_the_day_count_state(engine):
    """40 endpoints x 20 days (tests/test_gpu_state_drop.py's shape), values whose pairwise and sequential sums differ; even keys are
    ingress endpoints, odd keys egress ones"""
    K, days = 40, 20
    rng = np.random.default_rng(11)
    vals = []
    for key in range(K):
        for _ in range(50):
            v = drop_values(rng, days)
            v[:] = (v >> np.uint64(10)) | np.uint64(1 << 49)
            if key % 5 == 0:
                v[7] |= np.uint64(1 << 61)                  # a day far above mean + 3 std
            if order_sensitive(v):
                break
        assert order_sensitive(v)
        vals.append(v)
    k = np.repeat(np.arange(K, dtype=U64), days)
    t = np.tile(D_BASE + DAY * np.arange(days, dtype=np.int64), K)
    v = np.concatenate(vals)
    st = new_state(engine, K, SER | TIMES)
    engine.run_stream(st, k, t, v, agg_flow="svc", value_op="sum")
    W = window(st)
    assert np.array_equal(W[0], k) and np.array_equal(W[1], t) and np.array_equal(W[2], v)
    snap = snapshot(st)
    direction = np.arange(K) % 2
    for name, keep in (("ingress", direction == 0), ("egress", direction == 1), ("every third key", np.arange(K) % 3 == 0), ("none", np.zeros(K, bool))):
        keep = keep.astype(np.uint8)
        for win in ((0, 0, 0), (D_BASE + 3 * DAY, D_BASE + 17 * DAY, 0), (0, 0, 9)):
            m = in_window(W[0], W[1], *win) & (keep[W[0].astype(np.int64)] != 0)
            Wm = tuple(c[m] for c in W)
            for emit_all in (True, False):
                tag = (name, win, emit_all)
                got = engine.drop_state_keys(st, keep, *win, emit_all=emit_all)
                assert_same(snapshot(st), snap, tag)
                full = rows_of(engine.drop_state(st, *win, emit_all=emit_all))
                sel = keep[full["key_id"].astype(np.int64)] != 0
                assert_rows(rows_of(got), {f: a[sel] for f, a in full.items()}, (tag, "R1"))
                want, no_result = drop_oracle_rows(Wm, emit_all=emit_all)
                assert_rows(rows_of(got), want, (tag, "oracle"))
                gs = got.stats
                assert gs["rows_in"] == gs["rows_used"] == gs["n_points"] == Wm[0].size and gs["keys_no_result"] == no_result, tag
                assert gs["n_keys"] == np.unique(Wm[0]).size, tag
                if Wm[0].size == 0:
                    assert got.n_rows == 0 and gs["t0"] == 0
                    continue
                ref = engine.run("DROP", Wm[0], Wm[1], Wm[2], K, agg_flow="svc", value_op="sum", emit_all=emit_all)
                assert_rows(rows_of(got), rows_of(ref), (tag, "R2"))
                for f in ("n_keys", "n_points", "n_anomalies", "keys_no_result", "t0"):
                    assert gs[f] == ref.stats[f], (tag, f)
                if name == "ingress" and not emit_all and win == (0, 0, 0):
                    assert got.n_rows > 0 and (np.asarray(got["key_id"]) % 2 == 0).all()
    # parameters away from their defaults, and the mask from a device slice
    keep = (np.arange(K) % 3 == 0).astype(np.uint8)
    m = keep[W[0].astype(np.int64)] != 0
    got = engine.drop_state_keys(st, keep, nsigma=1.5, min_samples=21, emit_all=True)
    assert got.n_rows == 0 and got.stats["keys_no_result"] == int(keep.sum())               # 20 points a key < min_samples
    got = engine.drop_state_keys(st, keep, nsigma=1.5, min_samples=5)
    assert_rows(rows_of(got), drop_oracle_rows(tuple(c[m] for c in W), nsigma=1.5, ms=5)[0], "nsigma 1.5")
    assert got.n_rows > 0
    st.close()


# ---- 8. flags and parameters; the mask's memory ----
def test_parameters_away_from_their_defaults_and_the_mask_in_either_memory(engine):
    lens = 6 + (np.arange(90) * 11) % 35
    st, W = make_state(engine, lens, seed=31, spread=1800)
    K = lens.size
    snap = snapshot(st)
    keep = mask_of("a random half", K, seed=1)
    params = {"EWMA": {"alpha": 0.2}, "DBSCAN": {"eps": 1.5e8, "min_samples": 3}, "ARIMA": {"maxiter": 3}}
    lo, hi = int(W[1].min()), int(W[1].max())
    win = (lo + 200, hi - 200, 0)
    got = check_keys(engine, st, W, keep, win, algos=("EWMA", "DBSCAN", "ARIMA"), what="parameters", params=params, snap=snap)
    dflt = check_keys(engine, st, W, keep, win, algos=("EWMA", "DBSCAN"), what="defaults", snap=snap)
    for algo, field in (("EWMA", "algo_calc"), ("DBSCAN", "anomaly")):     # the parameters reached the detector: other values, other verdicts
        assert not np.array_equal(rows_of(got[(algo, True)])[field], rows_of(dflt[(algo, True)])[field]), algo
        assert "anomaly" in rows_of(got[(algo, True)]) and "anomaly" not in rows_of(got[(algo, False)])
    # the mask from host memory, from a device array and from a device slice offset by 1 byte: the same rows
    blob = np.zeros((K + 1 + 7) // 8 * 8, np.uint8)
    blob[1:1 + K] = keep * 7                                  # (any non-zero byte selects)
    dev = DeviceArray.from_host(engine, blob.view(np.uint64))
    aligned = DeviceArray.from_host(engine, np.concatenate([keep, np.zeros(-K % 8, np.uint8)]).view(np.uint64)).view(0, K, np.uint8)
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        host = rows_of(got[(algo, True)])
        for arg in (dev.view(1, K, np.uint8), aligned, keep.astype(bool), (keep * 255).astype(np.uint8)):
            again = engine.run_state_keys(st, arg, *win, algo=algo, emit_all=True, **params[algo])
            assert_rows(rows_of(again), host, (algo, type(arg)))
        on_dev = engine.run_state_keys(st, dev.view(1, K, np.uint8), *win, algo=algo, emit_all=True, out="device", **params[algo])
        assert on_dev.memory == "device"
        assert_rows(rows_of(on_dev), host, (algo, "device result"))
        on_dev.close()
    assert_same(snapshot(st), snap)
    st.close()


# ---- 9. after merge, trim and compact, the mask passed through remap ----
def test_after_merge_trim_and_compact(engine):
    K = 120
    k, t, v = orc.synth_rows(0, 200 * K, K, 48)
    dies = (k % np.uint64(4) == 3) & (t > np.median(t))       # every fourth key falls silent half way
    k, t, v = k[~dies], t[~dies], v[~dies]
    part = np.random.default_rng(5).integers(0, 4, size=k.size)
    st = new_state(engine, K)
    for p in (2, 0, 3, 1):                                    # out-of-order batches, rows of one group split over batches
        engine.merge_stream(st, k[part == p], t[part == p], v[part == p], agg_flow="svc", value_op="sum")
    keep = mask_of("a random half", K, seed=2)
    W = window(st)
    lo, hi = int(W[1].min()), int(W[1].max())
    check_keys(engine, st, W, keep, (lo + 600, hi - 300, 0), what="merged")
    check_keys(engine, st, W, keep, what="merged, unwindowed", emits=(True,))
    st.trim(keep_from=lo + 900)
    st.trim(keep_points=30)
    W = window(st)
    assert W[0].size and np.bincount(W[0].astype(np.int64), minlength=K).max() <= 30
    check_keys(engine, st, W, keep, (0, hi - 300, 0), what="trimmed")
    # retire the keys whose newest point is old: the survivors are renumbered, the mask follows through remap
    last = np.array([W[1][W[0] == key].max() if (W[0] == key).any() else 0 for key in range(K)])
    cut = int(last.max())
    assert 0 < (last < cut).sum() < K                         # the silent keys' newest point is older than the others'
    remap, stats = st.compact(retire_before=cut)
    remap = np.asarray(remap)
    alive = remap != np.uint64(_capi.TAD_KEY_SKIP)
    assert 0 < alive.sum() < K and st.num_keys == alive.sum()
    new_keep = np.zeros(st.num_keys, np.uint8)
    new_keep[remap[alive].astype(np.int64)] = keep[alive]
    assert 0 < new_keep.sum() < new_keep.size
    W2 = window(st)
    check_keys(engine, st, W2, new_keep, (0, hi - 300, 0), what="compacted")
    with pytest.raises(TadError) as ei:                       # the mask of before the compact is stale: refused, not read short
        engine.run_state_keys(st, keep)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "key_keep" in ei.value.message
    st.close()


# ---- 10. refusals ----
def raw_call(engine, st, fn, keep_ptr, keep_len, key_memory=_capi.TAD_MEM_HOST, from_t=0, to_t=0, **job):
    j = _capi.Job(**job)
    res = C.POINTER(_capi.Result)()
    rc = getattr(engine._lib, fn)(engine._h, st._h, C.byref(j), from_t, to_t, 0, keep_ptr, keep_len, key_memory, _capi.TAD_MEM_HOST, C.byref(res))
    if rc == _capi.TAD_OK:
        engine._lib.tad_result_free(engine._h, res)
    else:
        assert not res
    return rc


def test_refusals(engine):
    lens = np.array([20, 30, 25, 40, 8])
    st, W = make_state(engine, lens, seed=6)
    K = lens.size
    snap = snapshot(st)
    keep = np.array([1, 0, 1, 1, 0], np.uint8)
    bad = _capi.TAD_ERR_INVALID_ARGUMENT
    a, b = T_BASE + 5, T_BASE + 20
    run, drop, DROP = "tad_run_state_keys", "tad_drop_state_keys", _capi.TAD_ALGO["DROP"]
    assert raw_call(engine, st, run, keep.ctypes.data, K, algo=0) == _capi.TAD_OK
    assert raw_call(engine, st, drop, keep.ctypes.data, K, algo=DROP) == _capi.TAD_OK
    assert raw_call(engine, st, run, None, 0, algo=0) == _capi.TAD_OK                                  # no mask: the window call
    for fn, algo in ((run, 0), (drop, DROP)):
        for name, args in {"short": (keep.ctypes.data, K - 1), "long": (keep.ctypes.data, K + 1), "zero length": (keep.ctypes.data, 0),
                           "NULL with a length": (None, K)}.items():
            assert raw_call(engine, st, fn, *args, algo=algo) == bad, (fn, name)
            assert b"key_keep" in engine._lib.tad_last_error(engine._h), (fn, name)
        assert raw_call(engine, st, fn, keep.ctypes.data, K, key_memory=5, algo=algo) == bad
        # everything the window calls refuse
        assert raw_call(engine, st, fn, keep.ctypes.data, K, algo=DROP if fn == run else 0) == bad       # DROP on run, EWMA on drop
        assert raw_call(engine, st, fn, keep.ctypes.data, K, from_t=b, to_t=a, algo=algo) == bad         # from_t > to_t
        assert raw_call(engine, st, fn, keep.ctypes.data, K, from_t=a, to_t=a, algo=algo) == _capi.TAD_OK
        for job in (dict(start_time=T_BASE), dict(end_time=T_BASE + 9), dict(flags=_capi.TAD_FLAG_KEY_U32), dict(flags=_capi.TAD_FLAG_TIME_U32)):
            assert raw_call(engine, st, fn, keep.ctypes.data, K, algo=algo, **job) == bad, (fn, job)
        assert_same(snapshot(st), snap, fn)
    for fn, algo in ((run, 0), (drop, DROP)):                 # without a mask the refusals are the same, under the call's own name
        assert raw_call(engine, st, fn, None, 0, from_t=b, to_t=a, algo=algo) == bad
        assert fn.encode() + b": from_t is later than to_t" in engine._lib.tad_last_error(engine._h), fn
        assert raw_call(engine, st, fn, None, 0, algo=algo, start_time=T_BASE) == bad and fn.encode() in engine._lib.tad_last_error(engine._h)
    assert raw_call(engine, st, drop, None, 0, algo=DROP) == _capi.TAD_OK
    assert raw_call(engine, st, run, keep.ctypes.data, K, algo=0, ewma_alpha=1.5) == bad
    assert raw_call(engine, st, drop, keep.ctypes.data, K, algo=DROP, drop_nsigma=-1.0) == bad
    # stale times: the series imported, its times not yet
    stale = new_state(engine, K)
    stale.load(snap["state"])
    stale.load_history(*snap["history"])
    stale.load_series(*snap["series"])
    for call in (lambda: engine.run_state_keys(stale, keep), lambda: engine.drop_state_keys(stale, keep)):
        with pytest.raises(TadError) as ei:
            call()
        assert ei.value.code == bad
    stale.load_times(snap["times"])
    assert_rows(rows_of(engine.run_state_keys(stale, keep, emit_all=True)), rows_of(engine.run_state_keys(st, keep, emit_all=True)), "times imported")
    stale.close()
    # states that lack what the algorithm needs
    plain = engine.state_create(K)
    with pytest.raises(TadError):
        engine.run_state_keys(plain, keep)
    plain.close()
    nohist = new_state(engine, K, SER | TIMES)
    with pytest.raises(TadError):
        engine.run_state_keys(nohist, keep, algo="DBSCAN")
    assert engine.run_state_keys(nohist, keep, emit_all=True).n_rows == 0            # an empty state: no rows, no error
    assert engine.drop_state_keys(nohist, keep, emit_all=True).n_rows == 0
    nohist.close()
    assert_same(snapshot(st), snap)
    st.close()
