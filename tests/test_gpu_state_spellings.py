"""GPU: the five read-only jobs on a streaming state are one call (tad_capi_view.cpp: view_call), so every way of spelling the same
window gives the same answer: tad_run_state, tad_run_state_window and tad_run_state_keys for EWMA, DBSCAN and ARIMA, tad_drop_state and
tad_drop_state_keys for DROP.  The comparisons are between calls, never against a tolerance: rows bit for bit (floats as uint64),
n_anomalies and host_syncs equal.  One state serves every test and no call changes it: five keys of 20, 30, 25, 40 and 600 points — the
last above the 512 points from which a key is walked cooperatively (tad_internal.h kCoopMinT), the rest lane-sized."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import _capi
from theia_amd.engine import DeviceArray
from state_helpers import T_BASE, bits, rows_of

pytestmark = pytest.mark.gpu

LENS = (20, 30, 25, 40, 600)
ALGOS = ("EWMA", "DBSCAN", "ARIMA", "DROP")
RUN_CALLS = ("tad_run_state", "tad_run_state_window", "tad_run_state_keys")
DROP_CALLS = ("tad_drop_state", "tad_drop_state_keys")
EWMA, DROP = _capi.TAD_ALGO["EWMA"], _capi.TAD_ALGO["DROP"]

# tad_last_error after the refusals that every one of the five calls makes (start_time != 0, an algorithm of the other family) and after
# from_t > to_t on the four calls with a window: recorded from the library of before the calls shared one path, byte for byte.
REFUSALS = {
    ("tad_run_state", "start_time"): b"tad_run_state: start_time / end_time must be 0: the window is what the state holds (tad_state_trim narrows it)",
    ("tad_run_state", "family"): b"tad_run_state: the algorithm must be EWMA, DBSCAN or ARIMA (DROP: tad_drop_state)",
    ("tad_run_state_window", "start_time"): b"tad_run_state_window: start_time / end_time must be 0: the window is from_t / to_t / keep_points",
    ("tad_run_state_window", "family"): b"tad_run_state_window: the algorithm must be EWMA, DBSCAN or ARIMA (DROP: tad_drop_state)",
    ("tad_run_state_window", "from_t"): b"tad_run_state_window: from_t is later than to_t",
    ("tad_run_state_keys", "start_time"): b"tad_run_state_keys: start_time / end_time must be 0: the window is from_t / to_t / keep_points",
    ("tad_run_state_keys", "family"): b"tad_run_state_keys: the algorithm must be EWMA, DBSCAN or ARIMA (DROP: tad_drop_state)",
    ("tad_run_state_keys", "from_t"): b"tad_run_state_keys: from_t is later than to_t",
    ("tad_drop_state", "start_time"): b"tad_drop_state: start_time / end_time must be 0: the window is from_t / to_t / keep_points",
    ("tad_drop_state", "family"): b"tad_drop_state: the algorithm must be DROP (tad_run_state_window judges EWMA, DBSCAN and ARIMA)",
    ("tad_drop_state", "from_t"): b"tad_drop_state: from_t is later than to_t",
    ("tad_drop_state_keys", "start_time"): b"tad_drop_state_keys: start_time / end_time must be 0: the window is from_t / to_t / keep_points",
    ("tad_drop_state_keys", "family"): b"tad_drop_state_keys: the algorithm must be DROP (tad_run_state_keys judges EWMA, DBSCAN and ARIMA)",
    ("tad_drop_state_keys", "from_t"): b"tad_drop_state_keys: from_t is later than to_t",
}


def assert_same_answer(got, want, syncs, what):
    """two spellings of one job: the same rows bit for bit, the same n_anomalies, the host synchronisations the path is known by"""
    g, w = rows_of(got), rows_of(want)
    assert set(g) == set(w) and got.n_rows == want.n_rows, (what, got.n_rows, want.n_rows)
    for f in w:
        assert np.array_equal(bits(g[f]), bits(w[f])), (what, f)
    assert got.stats["n_anomalies"] == want.stats["n_anomalies"], what
    assert got.stats["host_syncs"] == want.stats["host_syncs"] == syncs, (what, got.stats["host_syncs"], want.stats["host_syncs"])


@pytest.fixture(scope="module")
def state(engine):
    """-> (state, window): key k holds LENS[k] points at the seconds T_BASE + 0, 1, 2 ..., seeded values around a base with two points far
    off per key; the window cuts every key (from the 5th second the state holds to the 5th from its last, the newest 10 points of those)"""
    rng = np.random.default_rng(20)
    k = np.repeat(np.arange(len(LENS), dtype=np.uint64), LENS)
    t = np.concatenate([T_BASE + np.arange(n, dtype=np.int64) for n in LENS])
    v = np.concatenate([3_000_000_000 + rng.integers(-300_000_000, 300_000_000, size=n) for n in LENS])
    for start, n in zip(np.cumsum((0,) + LENS[:-1]), LENS):
        v[start + n // 3] *= 3
        v[start + n - 2] //= 4
    o = rng.permutation(k.size)
    st = engine.state_create(len(LENS), history=True, series=True, times=True)
    engine.run_stream(st, np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o].astype(np.uint64)), value_op="max")
    assert np.array_equal(st.export_series()[0], np.asarray(LENS, dtype=np.uint64))
    seconds = np.unique(st.export_times())
    win = (int(seconds[4]), int(seconds[-5]), 10)
    assert all(n > 10 + 4 for n in LENS)                              # from_t and keep_points both cut every key
    yield st, win
    st.close()


def window_call(engine, st, algo, win, emit_all):
    if algo == "DROP":
        return engine.drop_state(st, *win, emit_all=emit_all)
    return engine.run_state_window(st, *win, algo=algo, emit_all=emit_all)


def keys_call(engine, st, algo, keep, win, emit_all):
    if algo == "DROP":
        return engine.drop_state_keys(st, keep, *win, emit_all=emit_all)
    return engine.run_state_keys(st, keep, *win, algo=algo, emit_all=emit_all)


@pytest.mark.parametrize("emit_all", [False, True], ids=["anomalies", "emit-all"])
@pytest.mark.parametrize("algo", ALGOS)
def test_the_whole_state_in_every_spelling(engine, state, algo, emit_all):
    st, _ = state
    ref = window_call(engine, st, algo, (0, 0, 0), emit_all)
    assert ref.n_rows == (sum(LENS) if emit_all else ref.stats["n_anomalies"])
    assert_same_answer(keys_call(engine, st, algo, None, (0, 0, 0), emit_all), ref, 2, (algo, "keys, no mask"))
    if algo != "DROP":
        assert_same_answer(engine.run_state(st, algo=algo, emit_all=emit_all), ref, 2, (algo, "run_state"))


@pytest.mark.parametrize("emit_all", [False, True], ids=["anomalies", "emit-all"])
@pytest.mark.parametrize("algo", ALGOS)
def test_one_window_in_every_spelling(engine, state, algo, emit_all):
    st, win = state
    ref = window_call(engine, st, algo, win, emit_all)
    assert ref.stats["n_points"] == 10 * len(LENS)
    assert_same_answer(keys_call(engine, st, algo, None, win, emit_all), ref, 3, (algo, "keys, no mask"))
    ones = np.ones(len(LENS), np.uint8)
    assert_same_answer(keys_call(engine, st, algo, ones, win, emit_all), ref, 3, (algo, "all ones, host"))
    dev = DeviceArray.from_host(engine, ones)
    assert_same_answer(keys_call(engine, st, algo, dev, win, emit_all), ref, 3, (algo, "all ones, device"))
    dev.free()


@pytest.mark.parametrize("emit_all", [False, True], ids=["anomalies", "emit-all"])
@pytest.mark.parametrize("algo", ALGOS)
def test_a_mixed_mask_selects_the_window_calls_rows(engine, state, algo, emit_all):
    st, win = state
    keep = np.array([1, 0, 1, 0, 1], np.uint8)
    want = rows_of(window_call(engine, st, algo, win, emit_all))
    sel = keep[want["key_id"].astype(np.int64)] != 0
    got = rows_of(keys_call(engine, st, algo, keep, win, emit_all))
    assert set(got) == set(want) and got["key_id"].size == int(sel.sum())
    if emit_all:
        assert got["key_id"].size == 10 * int(keep.sum())
    for f in want:
        assert np.array_equal(bits(got[f]), bits(want[f][sel])), (algo, f)


def refusal(engine, st, fn, job, from_t=0, to_t=0):
    """-> tad_last_error after the call `fn` refused `job` (with the window from_t / to_t where the call has one)"""
    res = C.POINTER(_capi.Result)()
    args = () if fn == "tad_run_state" else (from_t, to_t, 0)
    if fn.endswith("_keys"):
        args += (None, 0, _capi.TAD_MEM_HOST)
    rc = getattr(engine._lib, fn)(engine._h, st._h, C.byref(job), *args, _capi.TAD_MEM_HOST, C.byref(res))
    assert rc == _capi.TAD_ERR_INVALID_ARGUMENT and not res, (fn, rc)
    return bytes(engine._lib.tad_last_error(engine._h))


def test_the_refusals_every_call_shares_keep_their_text(engine, state):
    st, _ = state
    seen = {}
    for fn in RUN_CALLS + DROP_CALLS:
        own, other = (DROP, EWMA) if fn in DROP_CALLS else (EWMA, DROP)
        seen[fn, "start_time"] = refusal(engine, st, fn, _capi.Job(algo=own, start_time=T_BASE))
        seen[fn, "family"] = refusal(engine, st, fn, _capi.Job(algo=other))
        if fn != "tad_run_state":
            seen[fn, "from_t"] = refusal(engine, st, fn, _capi.Job(algo=own), from_t=T_BASE + 9, to_t=T_BASE + 3)
    assert sorted(seen) == sorted(REFUSALS)
    for case in sorted(REFUSALS):
        assert seen[case] == REFUSALS[case], (case, seen[case])
