"""What the TadState-level tests share: the constants of a state and its rows, how a state is created, exported (`snapshot`) and compared
(`assert_same`), how result rows are compared (`assert_rows`), the generators of batches, the host oracles of a window of a state, and the
bucket-edge tables.  Nothing here knows a host model (state_model.py and its kin import this module); what drives a state next to a model
is in state_drivers.py.  The asserts carry their own messages: pytest does not rewrite a module that is no test module."""
import ctypes as C

import numpy as np

from oracle import drop_oracle as dro
from oracle import tad_oracle as orc
from theia_amd import _capi

T_BASE = 1660202814
U64 = np.uint64
I64 = np.int64
SKIP = np.uint64((1 << 64) - 1)
ROW_FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")
STATE_FIELDS = ("n", "avg", "m2", "ewma", "last_t")
COUNTERS = ("n_keys", "n_points", "n_anomalies", "keys_no_result", "arima_fits", "arima_nan_fits", "kalman_steps")
HIST_CHUNK = 2048             # tad_internal.h   kHistChunk
COOP_MIN_T = 512              # tad_internal.h   kCoopMinT
HIST, SER, TIMES = 1, 2, 8     # TAD_STATE_HISTORY, TAD_STATE_SERIES, TAD_STATE_TIMES
ALL = HIST | SER | TIMES       # 11


def bits(a):
    """the array as it is compared: 8-byte items by their bit patterns (a NaN equals itself, -0.0 differs from 0.0)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def rows_of(res):
    """a TadResult's rows as a dict of host arrays, with the verdict column where the call asked for every point"""
    d = {f: np.asarray(res[f]) for f in ROW_FIELDS}
    if "anomaly" in res.to_host():
        d["anomaly"] = np.asarray(res["anomaly"])
    return d


def assert_rows(got, want, what=""):
    """"the rows are equal": the same fields, the same number of rows, every field equal by bits"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    assert got["key_id"].size == want["key_id"].size, (what, got["key_id"].size, want["key_id"].size)
    for f in want:
        assert np.array_equal(bits(got[f]), bits(want[f])), (what, f)


def new_state(engine, K, flags=ALL):
    return engine.state_create(K, history=bool(flags & HIST), series=bool(flags & SER), times=bool(flags & TIMES))


def snapshot(st):
    """everything a state holds, on the host; a part the state was created without is None, and so are the times of a state without points
    (tad_state_export_times writes nothing then)"""
    return {"state": st.export(), "history": st.export_history() if st.history else None,
            "series": st.export_series() if st.series else None, "times": st.export_times() if st.times and st.series_points() else None}


def assert_same(a, b, what=""):
    """"the state is unchanged" / "the states are equal", on two snapshots: every moment by bits; history, series and times present on
    both sides or on neither, and equal where present"""
    for f in STATE_FIELDS:
        assert np.array_equal(bits(a["state"][f]), bits(b["state"][f])), (what, f)
    for part in ("history", "series"):
        assert (a[part] is None) == (b[part] is None), (what, part)
        if a[part] is not None:
            assert np.array_equal(a[part][0], b[part][0]) and np.array_equal(a[part][1], b[part][1]), (what, part)
    assert (a["times"] is None) == (b["times"] is None), (what, "times")
    if a["times"] is not None:
        assert np.array_equal(a["times"], b["times"]), (what, "times")


def assert_counts(stats, want, what=""):
    for f, v in want.items():
        assert stats[f] == v, (what, f, stats[f], v)


def expected_counts(prev_rows, batch, op, keep_from=0):
    """what the call's counters must say, from sets of (key, time) on the host"""
    pk, pt, _ = orc.stage0(*prev_rows, op) if prev_rows[0].size else (np.zeros(0, U64), np.zeros(0, np.int64), None)
    bk, bt, _ = orc.stage0(*batch, op)
    old = set(zip(pk.tolist(), pt.tolist()))
    last = {}
    for k, t in zip(pk.tolist(), pt.tolist()):
        last[k] = t                    # (key, time) order: the last one wins
    c = {"batch_points": int(bk.size), "points_too_old": 0, "points_appended": 0, "points_inserted": 0, "points_combined": 0}
    touched, replayed = set(), set()
    for k, t in zip(bk.tolist(), bt.tolist()):
        if keep_from and t < keep_from:
            c["points_too_old"] += 1
            continue
        touched.add(k)
        if (k, t) in old:
            c["points_combined"] += 1
            replayed.add(k)
        elif k not in last or t > last[k]:
            c["points_appended"] += 1
        else:
            c["points_inserted"] += 1
            replayed.add(k)
    c["keys_touched"], c["keys_replayed"] = len(touched), len(replayed)
    return c


def raw_run_state(engine, st, **job):
    j = _capi.Job(**job)
    res = C.POINTER(_capi.Result)()
    rc = engine._lib.tad_run_state(engine._h, st._h, C.byref(j), _capi.TAD_MEM_HOST, C.byref(res))
    if rc == _capi.TAD_OK:
        engine._lib.tad_result_free(engine._h, res)
    else:
        assert not res, ("a refused tad_run_state left a result", rc)
    return rc


def minute_batches(n_rows, K, T, cuts, pod=False):
    k, t, v = orc.synth_rows(0, n_rows, K, T)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    edges = (0,) + tuple(cuts) + (T,)
    k2 = ((k + np.uint64(7)) % np.uint64(K)).astype(np.uint64)
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (bucket >= lo) & (bucket < hi)
        out.append((k[sel], t[sel], v[sel]) + ((k2[sel],) if pod else ()))
    return out


def second_batches(K, n_batches, width, pts_per_batch, seed, lifetimes=False):
    """second-resolution rows (two per point) in batches of `width` seconds; every key has exactly pts_per_batch points in every batch
    it is alive in.  lifetimes: a third of the keys only in the first half, a third only in the last batches, the rest throughout."""
    rng = np.random.default_rng(seed)
    out = []
    base = 1_000_000_000 + (orc.mix64(np.arange(K, dtype=np.uint64) + np.uint64(5)) % np.uint64(3_000_000_000)).astype(np.int64)
    for b in range(n_batches):
        alive = np.ones(K, bool)
        if lifetimes:
            g = np.arange(K) % 3
            alive = (g == 2) | ((g == 0) & (b < n_batches // 2)) | ((g == 1) & (b >= n_batches - 2))
        ks = np.nonzero(alive)[0].astype(np.uint64)
        pk = np.repeat(ks, pts_per_batch)
        pt = np.concatenate([np.sort(rng.choice(width, pts_per_batch, replace=False)) for _ in ks]).astype(np.int64) + T_BASE + b * width
        k, t = np.repeat(pk, 2), np.repeat(pt, 2)
        v = (np.repeat(base[pk.astype(np.int64)], 2) + rng.integers(-300_000_000, 300_000_000, size=k.size)).astype(np.uint64)
        order = rng.permutation(k.size)
        out.append((k[order], t[order], v[order]))
    return out


def point_codes(k, t, k2=None):
    """(key, time) of the batch's points as one uint64 code (key << 32 | t - T_BASE + 2^31)"""
    ks = [np.asarray(k, np.uint64)] + ([np.asarray(k2, np.uint64)] if k2 is not None else [])
    tt = (np.asarray(t, np.int64) - T_BASE + (1 << 31)).astype(np.uint64)
    out = [(kk[kk != SKIP] << np.uint64(32)) | tt[kk != SKIP] for kk in ks]
    return np.unique(np.concatenate(out))


def restrict(rows, codes):
    c = (rows["key_id"].astype(np.uint64) << np.uint64(32)) | (rows["flow_end_s"].astype(np.int64) - T_BASE + (1 << 31)).astype(np.uint64)
    sel = np.isin(c, codes)
    return {f: a[sel] for f, a in rows.items()}


def window(st):
    """W: one row per series point the state holds, (key, time, value) in (key, time) order"""
    ln, vals = st.export_series()
    keys = np.repeat(np.arange(st.num_keys, dtype=np.uint64), ln.astype(np.int64))
    return keys, st.export_times(), vals


def in_window(k, t, from_t=0, to_t=0, keep_points=0):
    """the mask of W' inside W (W in (key, time) order): the three rules of tad.h, in their order"""
    m = np.ones(k.size, bool)
    if from_t:
        m &= t >= from_t
    if to_t:
        m &= t < to_t
    if keep_points:
        idx = np.flatnonzero(m)
        kk = k[idx]
        from_end = np.searchsorted(kk, kk, side="right") - np.arange(kk.size)      # 1 = the key's newest point in the range
        m[idx[from_end > keep_points]] = False
    return m


def key_values(n, key, rng, ties=False):
    base = 1_000_000_000 + int(orc.mix64(np.array([key + 5], dtype=U64))[0] % U64(3_000_000_000))
    if ties:                                                  # two values only, the same for every key: ties across keys and inside them
        v = np.where(rng.random(n) < 0.3, 1_000_000_000, 1_000_000_000 + (1 << 23)).astype(np.int64)
    else:
        v = base + rng.integers(-300_000_000, 300_000_000, size=n)
    if n >= 6:                                                # two points far off: rows without the emit-all flag
        v[n // 3] = v[n // 3] * 3
        v[n - 2] = v[n - 2] // 4
    return v


def make_state(engine, lens, seed, starts=None, ties=(), history=True, spread=0):
    """-> (state, W).  spread: the points of a key at seeded seconds inside [0, spread) instead of consecutive ones"""
    rng = np.random.default_rng(seed)
    K = len(lens)
    ks, ts, vs = [], [], []
    for key, n in enumerate(lens):
        n = int(n)
        if n == 0:
            continue
        off = np.sort(rng.choice(spread, size=n, replace=False)) if spread else np.arange(n)
        ks.append(np.full(n, key, np.int64))
        ts.append(T_BASE + (int(starts[key]) if starts is not None else 0) + off.astype(np.int64))
        vs.append(key_values(n, key, rng, ties=key in ties))
    k, t, v = np.concatenate(ks).astype(U64), np.concatenate(ts), np.concatenate(vs).astype(U64)
    o = rng.permutation(k.size)
    st = new_state(engine, K, ALL if history else SER | TIMES)
    engine.run_stream(st, np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o]), value_op="max")
    assert np.array_equal(st.export_series()[0], np.asarray(lens).astype(U64)), ("make_state", "the segment lengths, from the state")
    return st, window(st)


def window_oracle_rows(W, m, algo, emit_all, **kw):
    """orc.run_job on W'': the rows the engine must return (EWMA, DBSCAN)"""
    k, t, v = W
    want = orc.run_job(algo, k[m], t[m], v[m], op="sum", **kw)
    if not emit_all:
        return {f: want[f] for f in ROW_FIELDS}
    pk, pt, pv = want["points"]
    sig = np.repeat(want["sigma"], np.diff(want["ptr"]))
    return {"key_id": pk, "flow_end_s": pt, "throughput": orc.u64_to_f64(pv), "algo_calc": want["calc_all"], "stddev": sig,
            "anomaly": want["anomaly_all"].astype(np.uint8)}


def drop_oracle_rows(W, nsigma=3.0, ms=3, emit_all=False, judged=None):
    """the rows tad_run(DROP) emits over W (in (key, time) order, one row per point), restricted to the points of mask `judged`;
    -> (rows, keys without a result among the keys with a judged point)"""
    k, t, v = W
    x = orc.u64_to_f64(v)
    judged = np.ones(k.size, bool) if judged is None else judged
    keys, first, cnt = np.unique(k, return_index=True, return_counts=True)
    sel, mean, std, verd = [], [], [], []
    no_result = 0
    for a, n in zip(first, cnt):
        j = judged[a:a + n]
        if not j.any():
            continue
        r = dro.drop_detection_series(x[a:a + n], nsigma, ms) if n >= 2 else None     # k_drop_detect: n >= min_samples && n >= 2
        if r is None:
            no_result += 1
            continue
        m, s, z = r
        idx = np.flatnonzero(j if emit_all else (j & z)) + a
        sel.append(idx)
        mean.append(np.full(idx.size, m))
        std.append(np.full(idx.size, s))
        verd.append(z[idx - a])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    sel = cat(sel, np.int64)
    rows = {"key_id": k[sel], "flow_end_s": t[sel], "throughput": x[sel], "algo_calc": cat(mean, np.float64), "stddev": cat(std, np.float64)}
    if emit_all:
        rows["anomaly"] = cat(verd, np.uint8)
    return rows, no_result


def order_sensitive(v):
    x = orc.u64_to_f64(v)
    s = dro.pairwise_sum(x)
    if s == np.cumsum(x)[-1]:
        return False
    sq = (s / x.size - x) ** 2
    return dro.pairwise_sum(sq) != np.cumsum(sq)[-1]


def pairwise_rows(A):
    """dro.pairwise_sum over every row of A (8 <= columns <= 128), vectorised over the rows: the same additions in the same order"""
    n = A.shape[1]
    assert 8 <= n <= 128, ("pairwise_rows", n)
    r = [A[:, j].copy() for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + A[:, i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + A[:, i]
        i += 1
    return res


EDGE_S = 8192                 # the bucket of the edge state: runs of up to 6145 consecutive seconds fit one bucket
EDGE_T0 = (T_BASE // EDGE_S) * EDGE_S
EDGE_RUNS = [
    [1, 63, 64, 65, 1, 2, 62, 66, 128, 129, 1],          # 0: runs around the 64-point slice, inside one chunk
    [3, 2044, 5, 9],                                     # 1: a run ending on element 2046, the next starting on 2047
    [3, 2045, 5, 9],                                     # 2: ending on 2047 (the chunk's last), the next starting on 2048 (a chunk's first)
    [3, 2046, 5, 9],                                     # 3: ending on 2048, starting on 2049
    [3, 2047, 5, 9],                                     # 4: ending on 2049, starting on 2050
    [2048, 2048, 7],                                     # 5: runs of exactly one chunk, aligned
    [5, 4097, 3],                                        # 6: one bucket over three chunks
    [2047, 6145, 2],                                     # 7: one bucket over four chunks, its head the last point of chunk 0
    [],                                                  # 8: empty
    [4097],                                              # 9: all points of the key in one bucket
    [1] * 70,                                            # 10: every point in a bucket of its own, over a slice edge
]


def run_times(runs, bucket_s, t0, skip=()):
    """times of a key whose consecutive runs have the given lengths: run j fills the first runs[j] seconds of bucket j (after `skip`ped
    bucket indices, which stay empty), buckets of bucket_s seconds from t0 (a bucket start) on"""
    out, b = [], 0
    for n in runs:
        while b in skip:
            b += 1
        assert 1 <= n <= bucket_s, ("run_times", n, bucket_s)
        out.append(t0 + b * bucket_s + np.arange(n, dtype=I64))
        b += 1
    return np.concatenate(out) if out else np.zeros(0, I64)


def wide_values(n, rng, top=0.0):
    """values of 50 .. 62 significant bits (a few thousand of them wrap a 64-bit sum); a share `top` of them with bit 63 set too"""
    bits_ = rng.integers(50, 63, size=n)
    v = (rng.integers(1 << 49, 1 << 50, size=n).astype(U64) << (bits_ - 50).astype(U64)) | U64(1)
    hi = rng.random(n) < top
    return np.where(hi, v | U64(1 << 63), v)
