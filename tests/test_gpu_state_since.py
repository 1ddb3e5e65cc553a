"""GPU: tad_run_state_since / tad_drop_state_since (include/tad.h) — judge the window, report from a time on.  The defining property: the
call returns the rows of tad_run_state_keys / tad_drop_state_keys with the same window and the EFFECTIVE mask (key_keep and key_since !=
TAD_NO_CHANGE), restricted to the points with flow_end_s >= since_t and >= key_since[key].  Every case makes that comparison: the keys
call's rows filtered on the host against the new call's, bit for bit, in order.  EWMA, DBSCAN and DROP are also checked against the
oracle on the judged table, filtered the same way.  Every case asserts its edge (which index the reported suffix starts at) from
host-side numbers first, and that the state is unchanged afterwards.  Helpers come from tests/test_gpu_state_keys.py."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadError, _capi
from theia_amd.engine import DeviceArray
from state_helpers import (I64, SER, TIMES, T_BASE, U64, assert_rows, assert_same, drop_oracle_rows, in_window, make_state, new_state, rows_of,
                           snapshot, window, window_oracle_rows)

pytestmark = pytest.mark.gpu

NO_CHANGE = _capi.TAD_NO_CHANGE
ALGOS = ("EWMA", "DBSCAN", "DROP")


def reported_mask(k, t, since_t, key_since):
    m = np.ones(k.size, bool)
    if since_t:
        m &= t >= since_t
    if key_since is not None:
        m &= t >= np.asarray(key_since, I64)[k.astype(I64)]
    return m


def keys_call(engine, st, algo, mask, win, emit_all, kw):
    if algo == "DROP":
        return engine.drop_state_keys(st, mask, *win, emit_all=emit_all, **kw)
    return engine.run_state_keys(st, mask, *win, algo=algo, emit_all=emit_all, **kw)


def since_call(engine, st, algo, since_t, key_since, keep, win, emit_all, kw):
    if algo == "DROP":
        return engine.drop_state_since(st, since_t, key_since, keep, *win, emit_all=emit_all, **kw)
    return engine.run_state_since(st, since_t, key_since, keep, *win, algo=algo, emit_all=emit_all, **kw)


def check_since(engine, st, W, since_t=0, key_since=None, keep=None, win=(0, 0, 0), algos=ALGOS, emits=(False, True), what="", params=None,
                first=None, since_arg=None, keep_arg=None, snap=None):
    """the new call against the keys call with the effective mask, filtered on the host; EWMA / DBSCAN / DROP against the oracle on the
    judged table.  first: {key: index} the host expects the reported suffix of that key to start at, inside its judged segment (asserted
    before the engine runs).  -> {(algo, emit_all): result}"""
    K = st.num_keys
    k, t, v = W
    ki = k.astype(I64)
    eff = np.ones(K, np.uint8) if keep is None else (np.asarray(keep) != 0).astype(np.uint8)
    if key_since is not None:
        eff &= (np.asarray(key_since, I64) != NO_CHANGE).astype(np.uint8)
    judged = in_window(k, t, *win) & (eff[ki] != 0)
    rep = judged & reported_mask(k, t, since_t, key_since)
    jk, jt, jv = k[judged], t[judged], v[judged]
    rep_j = rep[judged]
    for key, f in (first or {}).items():
        seg = rep_j[jk == key]
        at = int(np.flatnonzero(seg)[0]) if seg.any() else seg.size
        assert at == f, (what, "host", key, at, f)
        assert seg[f:].all() and not seg[:f].any(), (what, "host: the reported points are a suffix", key)
    snap = snap or snapshot(st)
    out = {}
    for algo in algos:
        kw = dict((params or {}).get(algo, {}))
        for emit_all in emits:
            tag = (what, algo, emit_all, win, since_t)
            full_res = keys_call(engine, st, algo, eff, win, emit_all, kw)
            full = rows_of(full_res)
            sel = reported_mask(full["key_id"], full["flow_end_s"], since_t, key_since)
            want = {f: a[sel] for f, a in full.items()}
            got = since_call(engine, st, algo, since_t, key_since if since_arg is None else since_arg, keep if keep_arg is None else keep_arg, win,
                             emit_all, kw)
            assert_same(snapshot(st), snap, (tag, "state changed"))
            assert_rows(rows_of(got), want, (tag, "the keys call, filtered"))
            gs, fs = got.stats, full_res.stats
            for f in ("rows_in", "rows_used", "n_points", "n_keys", "t0"):
                assert gs[f] == fs[f], (tag, f, gs[f], fs[f])
            assert gs["n_points"] == int(judged.sum()), (tag, gs["n_points"], int(judged.sum()))
            assert gs["n_anomalies"] == (int(want["anomaly"].sum()) if emit_all else int(sel.sum())), (tag, gs["n_anomalies"])
            if emit_all and algo in ("EWMA", "DBSCAN"):
                assert got.n_rows == int(rep.sum()), (tag, got.n_rows, int(rep.sum()))
            if judged.any() and (since_t or key_since is not None):
                # as built (tad.h): 2, one more when the window's size is read (bounds, a mask or a key_since on a non-empty state), one
                # more when the reported total is read (DBSCAN, ARIMA, DROP)
                bounds = any(win) or keep is not None or key_since is not None
                assert gs["host_syncs"] == 2 + (1 if bounds else 0) + (0 if algo == "EWMA" else 1), (tag, gs["host_syncs"], fs["host_syncs"])
            if algo == "DROP":
                orows, no_result = drop_oracle_rows((jk, jt, jv), kw.get("nsigma", 0.0) or 3.0, kw.get("min_samples", 0) or 3, emit_all, rep_j)
                assert_rows(rows_of(got), orows, (tag, "oracle"))
                assert gs["keys_no_result"] == no_result, (tag, gs["keys_no_result"], no_result)
            elif algo in ("EWMA", "DBSCAN") and judged.any():
                o = window_oracle_rows((jk, jt, jv), np.ones(jk.size, bool), algo, emit_all, **kw)
                osel = reported_mask(o["key_id"], o["flow_end_s"], since_t, key_since)
                assert_rows(rows_of(got), {f: a[osel] for f, a in o.items()}, (tag, "oracle"))
            out[(algo, emit_all)] = got
    return out


def time_of(W, key, index):
    """the time of point `index` of `key` in W"""
    return int(W[1][W[0] == key][index])


@pytest.fixture(scope="module")
def lane_state(engine):
    """70 keys of 1 .. 40 points at consecutive seconds (lengths around the 8-point chunk of the lane walk), key 7 empty"""
    lens = [1 + (7 * j + 3) % 40 for j in range(70)]
    lens[7] = 0
    lens[0], lens[1], lens[2], lens[3], lens[4], lens[5] = 1, 7, 8, 9, 16, 40
    st, W = make_state(engine, lens, seed=70)
    yield st, W, snapshot(st), lens
    st.close()


def test_since_t_on_a_point_behind_it_before_all_and_after_all(engine, lane_state):
    st, W, snap, lens = lane_state
    # every key starts at T_BASE: second T_BASE + 8 is point 8 of every key that has one
    check_since(engine, st, W, since_t=T_BASE + 8, what="on a point", snap=snap, first={5: 8, 3: 8, 2: 8, 1: 7, 0: 1, 4: 8})
    check_since(engine, st, W, since_t=T_BASE + 9, what="one second later", snap=snap, first={5: 9, 3: 9, 4: 9})
    check_since(engine, st, W, since_t=T_BASE - 5, what="before all points", snap=snap, first={5: 0, 0: 0, 1: 0})
    res = check_since(engine, st, W, since_t=T_BASE + 1000, what="after all points", snap=snap, first={5: 40, 0: 1})
    assert all(r.n_rows == 0 for r in res.values())


def test_no_since_at_all_is_the_keys_call_and_an_all_empty_report_has_no_rows(engine, lane_state):
    st, W, snap, lens = lane_state
    keep = (np.arange(len(lens)) % 3 != 0).astype(np.uint8)
    for algo in ALGOS + ("ARIMA",):
        for emit_all in (False, True):
            a = since_call(engine, st, algo, 0, None, keep, (T_BASE + 2, 0, 20), emit_all, {})
            b = keys_call(engine, st, algo, keep, (T_BASE + 2, 0, 20), emit_all, {})
            assert_rows(rows_of(a), rows_of(b), (algo, emit_all))
            for f in ("n_points", "n_keys", "t0", "n_anomalies", "keys_no_result", "arima_fits", "kalman_steps", "host_syncs", "pts_mean", "pts_m2"):
                assert a.stats[f] == b.stats[f], (algo, emit_all, f, a.stats[f], b.stats[f])
            none = since_call(engine, st, algo, 0, np.full(len(lens), NO_CHANGE, I64), keep, (0, 0, 0), emit_all, {})
            assert none.n_rows == 0 and none.stats["n_points"] == 0 and none.stats["n_keys"] == 0 and none.stats["n_anomalies"] == 0, (algo, emit_all)
    assert_same(snapshot(st), snap, "state changed")


@pytest.mark.parametrize("memory", ("host", "device"))
def test_per_key_since_mixing_no_change_the_first_and_the_last_time(engine, lane_state, memory):
    st, W, snap, lens = lane_state
    K = len(lens)
    ks = np.full(K, NO_CHANGE, I64)
    first = {}
    for j in range(K):
        if lens[j] == 0 or j % 4 == 3:
            continue                                           # NO_CHANGE (and the empty key)
        if j % 4 == 0:
            ks[j], first[j] = time_of(W, j, 0), 0              # the first time: the whole key
        elif j % 4 == 1:
            ks[j], first[j] = time_of(W, j, lens[j] - 1), lens[j] - 1   # the last time: one point
        else:
            ks[j], first[j] = time_of(W, j, lens[j] // 2) , lens[j] // 2
    arg = DeviceArray.from_host(engine, ks) if memory == "device" else None
    check_since(engine, st, W, key_since=ks, what=("mixed", memory), snap=snap, first=first, since_arg=arg)
    # both rules at once: the larger threshold wins per key
    check_since(engine, st, W, since_t=T_BASE + 5, key_since=ks, what=("mixed + since_t", memory), snap=snap, since_arg=arg,
                first={5: max(first.get(5, 0), 5)} if 5 in first else None)


def test_combined_with_the_window_and_a_key_mask(engine, lane_state):
    st, W, snap, lens = lane_state
    K = len(lens)
    keep = (np.arange(K) % 5 != 1).astype(np.uint8)
    ks = np.where(np.arange(K) % 6 == 2, NO_CHANGE, T_BASE + 3 + np.arange(K) % 11).astype(I64)
    for win in ((T_BASE + 2, T_BASE + 30, 0), (0, T_BASE + 25, 12), (T_BASE + 4, 0, 6), (0, 0, 9)):
        check_since(engine, st, W, since_t=T_BASE + 6, key_since=ks, keep=keep, win=win, what="window + mask", snap=snap,
                    keep_arg=DeviceArray.from_host(engine, np.resize(keep, (K + 7) // 8 * 8).view(np.uint64)) if win[2] == 9 else None,
                    since_arg=DeviceArray.from_host(engine, ks) if win[2] == 9 else None)


@pytest.mark.parametrize("emit", ("staged", "lane"))
def test_ewma_first_index_at_every_chunk_edge_of_lane_and_coop_keys(engine, emit):
    """first[k] at 0, 1, 63, 64, 65, len - 1 and len: on lane keys around the 8-point chunk (7, 8, 9 in the place of 63, 64, 65) and on
    coop keys of 511 (a lane key: below the 512 of kCoopMinT), 512, 513 and 576 points"""
    lens = [1, 7, 8, 9, 16, 17, 40, 511, 512, 513, 576]
    st, W = make_state(engine, lens, seed=5)
    snap = snapshot(st)
    K = len(lens)
    with engine.plan(ewma_emit=emit):
        for name, idx in (("0", lambda n: 0), ("1", lambda n: min(1, n)), ("7 | 63", lambda n: min(n, 7 if n <= 40 else 63)),
                          ("8 | 64", lambda n: min(n, 8 if n <= 40 else 64)), ("9 | 65", lambda n: min(n, 9 if n <= 40 else 65)),
                          ("len - 1", lambda n: n - 1), ("len", lambda n: n)):
            first = {j: idx(n) for j, n in enumerate(lens)}
            ks = np.array([time_of(W, j, first[j]) if first[j] < lens[j] else time_of(W, j, lens[j] - 1) + 1 for j in range(K)], I64)
            check_since(engine, st, W, key_since=ks, algos=("EWMA",), what=("first", name, emit), snap=snap, first=first)
    st.close()


def test_ewma_a_wavefront_of_64_keys_whose_rows_exceed_the_staged_capacity(engine):
    """64 keys of 40 points with two anomalies each and first = 3: 128 rows of one wavefront against a pinned capacity of 64 staged rows"""
    lens = [40] * 64 + [9] * 3
    st, W = make_state(engine, lens, seed=6)
    snap = snapshot(st)
    with engine.plan(ewma_emit="staged", ewma_emit_rows=64):
        res = check_since(engine, st, W, since_t=T_BASE + 3, algos=("EWMA",), what="past the staged capacity", snap=snap, first={0: 3, 63: 3, 64: 3})
    assert res[("EWMA", False)].n_rows > 64
    st.close()


def test_suffix_lengths_around_the_copy_chunk_and_a_suffix_that_starts_mid_chunk(engine):
    """the copy kernel packs a suffix in chunks of 2048 points: suffixes of 2047, 2048 and 2049 points, and one of 3000 that starts at
    index 1100 of a 4100-point key (two chunks, the second partial), beside short keys"""
    lens = [4100, 3, 2049, 0, 2048, 30]
    st, W = make_state(engine, lens, seed=8, history=True)
    snap = snapshot(st)
    for n_suffix in (2047, 2048, 2049, 3000):
        first = {0: 4100 - n_suffix, 2: max(0, 2049 - n_suffix), 4: max(0, 2048 - n_suffix), 1: 1, 5: 30}
        ks = np.array([time_of(W, 0, first[0]), time_of(W, 1, 1), time_of(W, 2, first[2]), NO_CHANGE, time_of(W, 4, first[4]),
                       time_of(W, 5, 29) + 1], I64)
        res = check_since(engine, st, W, key_since=ks, algos=("DBSCAN", "DROP"), what=("suffix", n_suffix), snap=snap, first=first)
        assert res[("DBSCAN", True)].n_rows == n_suffix + 2 + (2049 - first[2]) + (2048 - first[4])
    st.close()


def test_dbscan_on_the_sort_side_and_on_the_subtract_side_of_the_history_rule(engine):
    lens = [300, 40, 300, 7, 120]
    st, W = make_state(engine, lens, seed=9, ties=(1,))
    snap = snapshot(st)
    S = sum(lens)
    lib = engine._lib
    for win, side in (((0, 0, 20), 1), ((T_BASE + 3, 0, 0), 0)):
        P = int(in_window(W[0], W[1], *win).sum())
        assert lib.tad_window_history_by_sort(P, S) == side, (win, P, S)
        check_since(engine, st, W, since_t=T_BASE + 30, win=win, algos=("DBSCAN",), what=("history side", side), snap=snap)
        ks = np.array([time_of(W, 0, 290), NO_CHANGE, time_of(W, 2, 150), time_of(W, 3, 5), time_of(W, 4, 119)], I64)
        check_since(engine, st, W, key_since=ks, win=win, algos=("DBSCAN",), what=("history side, per key", side), snap=snap)
    st.close()


def test_drop_on_either_side_of_min_samples_and_of_512_points(engine):
    lens = [2, 3, 4, 9, 10, 11, 511, 512, 513, 1]
    st, W = make_state(engine, lens, seed=10, history=False)
    snap = snapshot(st)
    for ms in (0, 10):                                          # 3 (the default) and 10: keys 0 | 1, 2 and 3 | 4, 5 on either side
        ks = np.array([time_of(W, j, max(0, n - 2)) for j, n in enumerate(lens)], I64)
        res = check_since(engine, st, W, key_since=ks, algos=("DROP",), what=("drop_min_samples", ms), snap=snap, params={"DROP": {"min_samples": ms, "nsigma": 1.0}},
                          first={j: max(0, n - 2) for j, n in enumerate(lens)})
        assert res[("DROP", True)].stats["keys_no_result"] == sum(1 for n in lens if n < (ms or 3) or n < 2)
        check_since(engine, st, W, since_t=T_BASE + 1, algos=("DROP",), what=("since_t", ms), snap=snap, params={"DROP": {"min_samples": ms, "nsigma": 1.0}})
    st.close()


def arima_table(rng):
    """65 keys of at most 40 points: positive non-constant keys with n > 3, and among them keys of 1, 2, 3 points, a constant key and a
    key of zeros -> (lens, k, t, v, plain): plain = the positive non-constant keys with n > 3"""
    lens = [4 + (5 * j) % 37 for j in range(65)]
    lens[10], lens[20], lens[30] = 1, 2, 3
    ks, ts, vs = [], [], []
    for j, n in enumerate(lens):
        ks.append(np.full(n, j, U64))
        ts.append(T_BASE + np.arange(n, dtype=I64))
        vs.append((1_000_000 + rng.integers(0, 400_000, size=n)).astype(U64))
    vs[40][:] = 777_777                                      # constant
    vs[50][:] = 0                                            # non-positive
    plain = [j for j in range(65) if j not in (10, 20, 30, 40, 50)]
    return lens, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs), plain


def test_arima_reports_the_suffix_and_runs_the_suffixes_fits_only(engine):
    rng = np.random.default_rng(11)
    lens, k, t, v, plain = arima_table(rng)
    K = len(lens)
    st = new_state(engine, K, SER | TIMES)
    engine.run_stream(st, k, t, v, value_op="max")
    W = window(st)
    snap = snapshot(st)
    # first below 3 (0, 1, 2), at 3, inside and at len - 1, by key; keys of n <= 3, the constant and the zero key take first = 1
    first = {j: (0, 1, 2, 3, lens[j] // 2, lens[j] - 1)[j % 6] for j in plain}
    first.update({10: 0, 20: 1, 30: 1, 40: 1, 50: 1})
    ks = np.array([time_of(W, j, first[j]) for j in range(K)], I64)
    res = check_since(engine, st, W, key_since=ks, algos=("ARIMA",), what="arima", snap=snap, first=first)
    # the fits: on the plain keys alone, sum(n - max(first, 3)), strictly below the keys call's count
    mask = np.zeros(K, np.uint8)
    mask[plain] = 1
    for emit_all in (False, True):
        got = engine.run_state_since(st, 0, ks, mask, algo="ARIMA", emit_all=emit_all)
        full = engine.run_state_keys(st, mask, algo="ARIMA", emit_all=emit_all)
        want_fits = sum(lens[j] - max(first[j], 3) for j in plain)
        assert got.stats["arima_fits"] == want_fits, (emit_all, got.stats["arima_fits"], want_fits)
        assert want_fits < full.stats["arima_fits"] == sum(lens[j] - 3 for j in plain), (emit_all, full.stats["arima_fits"])
        assert got.stats["keys_no_result"] == 0 and got.stats["n_points"] == full.stats["n_points"]
    # keys without a result are counted among the keys with a reported point only
    only = np.full(K, NO_CHANGE, I64)
    only[[10, 40, 3]] = ks[[10, 40, 3]]
    got = engine.run_state_since(st, 0, only, None, algo="ARIMA")
    full = engine.run_state_keys(st, (only != NO_CHANGE).astype(np.uint8), algo="ARIMA")
    assert got.stats["keys_no_result"] == full.stats["keys_no_result"]
    assert_same(snapshot(st), snap, "state changed")
    st.close()


def test_refusals(engine, lane_state):
    st, W, snap, lens = lane_state
    K = len(lens)
    lib, inv = engine._lib, _capi.TAD_ERR_INVALID_ARGUMENT
    ks = np.full(K + 1, T_BASE, I64)
    keep = np.ones(K + 1, np.uint8)
    job = _capi.Job(algo=0)
    drop = _capi.Job(algo=3)
    res = C.POINTER(_capi.Result)()
    RW = _capi.ReportWindow
    bad = [RW(key_since=ks.ctypes.data, num_keys=K + 1), RW(key_since=ks.ctypes.data, num_keys=K - 1), RW(key_keep=keep.ctypes.data, num_keys=K + 1),
           RW(key_since=ks.ctypes.data, num_keys=K, key_memory=2), RW(key_since=ks.ctypes.data + 4, num_keys=K), RW(from_t=T_BASE + 9, to_t=T_BASE + 2)]
    for i, w in enumerate(bad):
        assert lib.tad_run_state_since(engine._h, st._h, C.byref(job), C.byref(w), 0, C.byref(res)) == inv, i
        assert lib.tad_drop_state_since(engine._h, st._h, C.byref(drop), C.byref(w), 0, C.byref(res)) == inv, i
        assert not res
    ok = RW(since_t=T_BASE + 3)
    assert lib.tad_run_state_since(engine._h, st._h, C.byref(job), None, 0, C.byref(res)) == inv
    assert lib.tad_run_state_since(engine._h, st._h, C.byref(drop), C.byref(ok), 0, C.byref(res)) == inv          # DROP is the other call's
    assert lib.tad_drop_state_since(engine._h, st._h, C.byref(job), C.byref(ok), 0, C.byref(res)) == inv
    assert lib.tad_run_state_since(engine._h, st._h, C.byref(_capi.Job(algo=0, start_time=5)), C.byref(ok), 0, C.byref(res)) == inv
    plain = engine.state_create(K)
    assert lib.tad_run_state_since(engine._h, plain._h, C.byref(job), C.byref(ok), 0, C.byref(res)) == inv
    plain.close()
    with pytest.raises(TadError):
        engine.run_state_since(st, key_since=np.zeros(K - 1, I64))
    assert_same(snapshot(st), snap, "refusals")
    # a num_keys that is not looked at: no array is given
    assert lib.tad_run_state_since(engine._h, st._h, C.byref(job), C.byref(RW(since_t=T_BASE + 3, num_keys=12345)), 0, C.byref(res)) == 0
    lib.tad_result_free(engine._h, res)
