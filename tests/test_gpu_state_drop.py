"""GPU: the drop detector on a streaming state (tad_drop_state / tad_drop_stream, include/tad.h).  The defining properties: tad_drop_state
returns exactly the rows tad_run(TAD_ALGO_DROP) returns for the table of the window's series points, bit for bit, and leaves the state as
it was; tad_drop_stream advances the state exactly as an EWMA stream batch does and emits, for the batch's points only, the rows
tad_run(DROP) over everything the state then holds emits for them.  Two references: oracle.drop_oracle (pandas' arithmetic, independent
of the engine) and the engine's own run("DROP") over the exported points.  Float columns are compared as uint64 bit patterns.

Values.  Small counts add up exactly in any order and would show nothing: every key's values carry 50 to 62 significant bits (below 2^62,
one row per (key, time), so Stage 0's sum cannot wrap), and a key is redrawn (at most 50 times) until both of its sums are
order-sensitive on the host — the pairwise sum differs from the left-to-right sum, for the values and for the squared deviations.  Keys
of at most 8 points are exempt (below 8 the order IS left to right, 8 is the fixed tree)."""
import numpy as np
import pytest

from oracle import drop_oracle as dro
from oracle import tad_oracle as orc
from theia_amd import TadError, _capi
from state_helpers import (HIST, ROW_FIELDS, SER, TIMES, assert_rows, assert_same, bits, drop_oracle_rows, in_window, new_state, order_sensitive,
                           pairwise_rows, rows_of, snapshot, window)

pytestmark = pytest.mark.gpu

T_BASE = 1660176000
DAY = 86400
COUNTERS = ("n_keys", "n_points", "n_anomalies", "keys_no_result")


def coop_min(K, P):
    """win_coop_min (tad_window.hip): the shortest series that takes a wavefront of its own"""
    return 512 if K <= 8192 else max(8 * (P // K + 1), 512)


# ---- values ----
def draw(rng, n):
    nb = rng.integers(50, 63, size=n)
    lo = np.left_shift(np.uint64(1), (nb - 1).astype(np.uint64))
    return lo + (rng.integers(0, 1 << 62, size=n, dtype=np.uint64) & (lo - np.uint64(1)))


def draw_key(rng, n, tweak=None):
    for _ in range(50):
        v = draw(rng, n)
        if tweak is not None:
            tweak(v)
        if n <= 8 or order_sensitive(v):
            return v
    return v


def outlier_at(*places):
    """a tweak for draw_keys: the values narrowed to 50 .. 52 bits, those at `places` raised to 62: points far above mean + 3 std"""
    def tweak(v):
        if v.size:
            v[:] = (v >> np.uint64(10)) | np.uint64(1 << 49)
            for i in places:
                v[i] |= np.uint64(1 << 61)
    return tweak


def draw_keys(lengths, seed=11, tweaks=None):
    rng = np.random.default_rng(seed)
    vals = [draw_key(rng, int(n), (tweaks or {}).get(i)) for i, n in enumerate(lengths)]
    for v in vals:
        assert v.size <= 8 or order_sensitive(v), v.size      # every key with n >= 9 is order-sensitive in both sums
        assert v.size == 0 or (int(v.max()) < 1 << 62 and int(v.min()) >= 1 << 49)
    return vals


def table(vals, starts=None):
    """one row per point: key k's points on consecutive days from day starts[k]; (key, time, value) in (key, time) order"""
    starts = starts if starts is not None else [0] * len(vals)
    k = np.concatenate([np.full(v.size, i, np.uint64) for i, v in enumerate(vals)]) if vals else np.zeros(0, np.uint64)
    t = np.concatenate([T_BASE + DAY * (int(s) + np.arange(v.size, dtype=np.int64)) for s, v in zip(starts, vals)])
    return k, t, np.concatenate(vals)


def fill(engine, st, W):
    engine.run_stream(st, W[0], W[1], W[2], agg_flow="svc", value_op="sum")


# ---- the oracle ----


def check_state(engine, st, K, win=(0, 0, 0), W=None, m=None, what="", **kw):
    """drop_state over the window equals the oracle and the engine's own run("DROP") over W' = W[m], with and without emit_all, and
    leaves the state as it was; returns the emit_all result"""
    W = W if W is not None else window(st)
    m = np.ones(W[0].size, bool) if m is None else m
    Wm = (W[0][m], W[1][m], W[2][m])
    okw = {"nsigma": kw.get("nsigma") or 3.0, "ms": kw.get("min_samples") or 3}
    snap = snapshot(st)
    out = None
    for emit_all in (True, False):
        got = engine.drop_state(st, *win, emit_all=emit_all, **kw)
        assert_same(snapshot(st), snap, (what, win, "state changed"))
        want, no_result = drop_oracle_rows(Wm, emit_all=emit_all, **okw)
        assert_rows(rows_of(got), want, (what, win, emit_all, kw, "oracle"))
        gs = got.stats
        assert gs["rows_in"] == gs["rows_used"] == gs["n_points"] == Wm[0].size, (what, win)
        assert (gs["stage0_path"], gs["stage0_attempts"], gs["step"], gs["n_buckets"]) == (0, 0, 0, 0)
        assert gs["keys_no_result"] == no_result and gs["n_keys"] == np.unique(Wm[0]).size, (what, win)
        if Wm[0].size == 0:
            assert got.n_rows == 0 and gs["t0"] == 0 and gs["n_anomalies"] == 0
            continue
        ref = engine.run("DROP", Wm[0], Wm[1], Wm[2], K, agg_flow="svc", value_op="sum", emit_all=emit_all,
                         drop_nsigma=kw.get("nsigma", 0.0), drop_min_samples=kw.get("min_samples", 0))
        assert_rows(rows_of(got), rows_of(ref), (what, win, emit_all, kw, "tad_run"))
        for f in COUNTERS + ("t0",):
            assert gs[f] == ref.stats[f], (what, win, f, gs[f], ref.stats[f])
        x = orc.u64_to_f64(Wm[2])
        assert abs(gs["pts_mean"] - x.mean()) <= 1e-12 * abs(x.mean()), (what, gs["pts_mean"], x.mean())
        if emit_all:
            out = got
    return out


# ---- 1. series-length edges ----
EDGES = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 135, 136, 137, 255, 256, 257, 263, 264, 265, 271, 272, 273,
         511, 512, 513, 1023, 1024, 1025]


def test_series_length_edges_lane_and_wavefront(engine):
    vals = draw_keys(EDGES)
    K = len(EDGES)
    cm = coop_min(K, sum(EDGES))
    assert cm == 512
    assert [n for n in EDGES if n >= cm] == [512, 513, 1023, 1024, 1025] and max(n for n in EDGES if n < cm) == 511     # wavefront | lane
    st = new_state(engine, K, SER | TIMES)
    W = table(vals)
    fill(engine, st, W)
    got = check_state(engine, st, K, W=W, what="edges")
    # every key with a result has its own mean / std in the rows, bit for bit the oracle's
    keys = np.unique(got["key_id"])
    assert keys.tolist() == [i for i, n in enumerate(EDGES) if n >= 3]
    for i in keys:
        mean, std = dro.drop_stats(orc.u64_to_f64(vals[i]))
        r = got["key_id"] == i
        assert r.sum() == EDGES[i] and np.all(bits(got["algo_calc"][r]) == bits(np.float64(mean))) and np.all(bits(got["stddev"][r]) == bits(np.float64(std)))
    st.close()


# ---- 2. one key in rounds of leaves ----
def test_long_keys_take_several_rounds_of_leaves(engine):
    lengths = [8191, 8192, 8193, 16385, 100000]
    vals = draw_keys(lengths)
    st = new_state(engine, 5, SER | TIMES)
    W = table(vals)
    fill(engine, st, W)
    check_state(engine, st, 5, W=W, what="rounds")
    st.close()


# ---- 3. the outlier rule above 8192 keys ----


def test_outlier_rule_above_8192_keys(engine):
    K, short = 8193, 64
    planted = {100: 519, 5000: 520}
    lengths = [planted.get(k, short) for k in range(K)]
    P = sum(lengths)
    cm = coop_min(K, P)
    assert P // K + 1 == 65 and cm == 520                  # key 100 (519 points) takes a lane, key 5000 (520) a wavefront
    rng = np.random.default_rng(11)
    A = draw(rng, K * short).reshape(K, short)             # the short keys, redrawn row by row until both sums are order-sensitive
    for _ in range(50):
        X = orc.u64_to_f64(A.ravel()).reshape(K, short)
        s = pairwise_rows(X)
        sq = (s[:, None] / short - X) ** 2
        bad = (s == np.cumsum(X, axis=1)[:, -1]) | (pairwise_rows(sq) == np.cumsum(sq, axis=1)[:, -1])
        if not bad.any():
            break
        A[bad] = draw(rng, int(bad.sum()) * short).reshape(-1, short)
    assert not bad.any()
    assert pairwise_rows(X[:3])[1] == dro.pairwise_sum(X[1])                     # the vectorised mirror is the oracle's sum
    big = dict(zip(planted, draw_keys(list(planted.values()))))
    vals = [big[k] if k in big else A[k] for k in range(K)]
    W = table(vals)
    st = new_state(engine, K, SER | TIMES)
    fill(engine, st, W)
    # the oracle, vectorised for the short keys
    X = orc.u64_to_f64(A.ravel()).reshape(K, short)
    mean = pairwise_rows(X) / short
    std = np.sqrt(pairwise_rows((mean[:, None] - X) ** 2) / (short - 1))
    for k, v in big.items():
        mean[k], std[k] = dro.drop_stats(orc.u64_to_f64(v))
    x = orc.u64_to_f64(W[2])
    mk, sk = mean[W[0].astype(np.int64)], std[W[0].astype(np.int64)]
    z = (x > mk + 3.0 * sk) | (x < mk - 3.0 * sk)
    snap = snapshot(st)
    got = engine.drop_state(st, emit_all=True)
    assert_rows(rows_of(got), {"key_id": W[0], "flow_end_s": W[1], "throughput": x, "algo_calc": mk, "stddev": sk, "anomaly": z.astype(np.uint8)}, "outlier")
    ref = engine.run("DROP", W[0], W[1], W[2], K, agg_flow="svc", value_op="sum", emit_all=True)
    assert_rows(rows_of(got), rows_of(ref), "outlier tad_run")
    plain = engine.drop_state(st)
    assert_rows(rows_of(plain), {f: rows_of(got)[f][z] for f in ROW_FIELDS}, "outlier plain")
    assert_same(snapshot(st), snap, "outlier: state changed")
    st.close()


# ---- 4. parameters ----
def test_parameters(engine):
    lengths = list(range(1, 13))
    # one point far out in every key: its z-score is (n - 1) / sqrt(n), between 2.5 and 3 for n = 9, 10 and above 3 for n = 11, 12
    vals = draw_keys(lengths, tweaks={i: outlier_at(n // 2) for i, n in enumerate(lengths)})
    K = len(lengths)
    st = new_state(engine, K, SER | TIMES)
    W = table(vals)
    fill(engine, st, W)
    default = rows_of(check_state(engine, st, K, W=W, what="defaults"))
    seen = []
    for nsigma, ms in ((2.5, 0), (1.0, 5), (3.0, 10), (0, 1), (0, 2)):
        got = rows_of(check_state(engine, st, K, W=W, what="params", nsigma=nsigma, min_samples=ms))
        keys = set(got["key_id"].tolist())
        assert 0 not in keys                                # a key of 1 point never has a result
        assert (1 in keys) == (ms in (1, 2))                # a key of 2 points has one with min_samples <= 2
        assert keys == {i for i, n in enumerate(lengths) if n >= max(ms or 3, 2)}
        same = got["key_id"].size == default["key_id"].size and all(np.array_equal(bits(got[f]), bits(default[f])) for f in got)
        seen.append(same)
    assert not any(seen), seen                              # every parameter set gives other rows than the defaults
    st.close()


# ---- 5. windows ----


def test_windows(engine):
    spans = [(0, 228), (0, 229), (50, 650), (101, 599), (0, 102), (0, 103), (200, 100), (0, 50), (610, 190), (0, 700)]     # (first day, points)
    vals = draw_keys([n for _, n in spans])
    K = len(spans)
    W = table(vals, [s for s, _ in spans])
    st = new_state(engine, K, SER | TIMES)
    fill(engine, st, W)
    day = lambda d: T_BASE + DAY * d
    inside_seen = set()
    for win in ((day(100), day(612), 0), (0, 0, 129), (0, 0, 128), (day(100), 0, 3), (day(100), day(612), 511)):
        m = in_window(W[0], W[1], *win)
        n_in = np.bincount(W[0][m].astype(np.int64), minlength=K)
        n_all = np.bincount(W[0].astype(np.int64), minlength=K)
        inside_seen |= set(n_in[(n_in > 0) & (n_in < n_all)].tolist())
        got = check_state(engine, st, K, win=win, W=W, m=m, what="window")
        assert got.stats["host_syncs"] == 3
    assert {2, 3, 128, 129, 511, 512} <= inside_seen, sorted(inside_seen)        # cut keys on both sides of every threshold
    # a window that leaves every key whole judges the state's own arrays: the bounds' synchronisation and no view
    whole = check_state(engine, st, K, win=(day(0), day(2000), 0), W=W, what="whole")
    assert whole.stats["host_syncs"] == 3 and whole.n_rows == W[0].size and check_state(engine, st, K, W=W).stats["host_syncs"] == 2
    # empty windows
    for win in ((day(300), day(300), 0), (day(5000), 0, 0)):
        check_state(engine, st, K, win=win, W=W, m=np.zeros(W[0].size, bool), what="empty")
    st.close()


# ---- 6. stream ----
PER_BATCH = [[2, 1, 4, 3], [128, 1, 7, 8], [600, 5, 5, 60], [0, 0, 9, 2], [20, 0, 0, 11], [0, 0, 0, 0]]


def batches(tweaks=None):
    """four batches of (key, time, value): key 0 crosses 2 -> 3 points and key 1 128 -> 129 in batch 1, key 2 is long (a wavefront from the
    start), key 3 appears in batch 2, key 4 is touched in batches 0 and 3 only, key 5 never"""
    vals = draw_keys([sum(p) for p in PER_BATCH], tweaks=tweaks)
    out, day0 = [], 0
    for b in range(4):
        part = [v[sum(p[:b]):sum(p[:b + 1])] for v, p in zip(vals, PER_BATCH)]
        out.append(table(part, [day0] * len(PER_BATCH)))
        day0 += max(p[b] for p in PER_BATCH)
    # batch 3 carries second-resolution times
    out[3] = (out[3][0], out[3][1] + (np.arange(out[3][1].size) * 7919) % 3600, out[3][2])
    return out, len(PER_BATCH)


def concat(parts):
    k, t, v = (np.concatenate([p[i] for p in parts]) for i in range(3))
    o = np.lexsort((t, k))
    return k[o], t[o], v[o]


@pytest.mark.parametrize("flags", [SER | TIMES, SER, HIST | SER | TIMES], ids=["series+times", "series-only", "history+series+times"])
def test_stream_batches(engine, flags):
    """after each batch: the rows are the oracle's over everything fed so far, restricted to the batch's points, and the state is bit
    for bit that of a twin fed the same batches through run_stream (EWMA)"""
    bs, K = batches()
    st, twin = new_state(engine, K, flags), new_state(engine, K, flags)
    kw = dict(agg_flow="svc", value_op="sum")
    first_rows = {}
    for b, B in enumerate(bs):
        if b == 2:                                           # a late row fails the batch and the state stays; the batch then goes on
            snap = snapshot(st)
            late = (np.append(B[0], np.uint64(2)), np.append(B[1], bs[0][1].min()), np.append(B[2], np.uint64(1 << 55)))
            with pytest.raises(TadError) as ei:
                engine.drop_stream(st, *late, **kw)
            assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT
            assert_same(snapshot(st), snap, "late row: state changed")
        if b == 3:                                           # second-resolution times forced through the sparse Stage 0
            with engine.plan(sparse="always"):
                got = engine.drop_stream(st, *B, emit_all=True, **kw)
                engine.run_stream(twin, *B, **kw)
            assert got.stats["stage0_path"] in (4, 8), got.stats["stage0_path"]
        else:
            got = engine.drop_stream(st, *B, emit_all=True, out="device" if b == 1 else "host", **kw)
            engine.run_stream(twin, *B, **kw)
        assert_same(snapshot(st), snapshot(twin), ("stream", b, "twin"))
        Wb = concat(bs[:b + 1])
        want, no_result = drop_oracle_rows(Wb, emit_all=True, judged=Wb[1] >= B[1].min())
        assert_rows(rows_of(got), want, ("stream", b))
        assert got.stats["keys_no_result"] == no_result and got.stats["n_points"] == B[0].size, (b, got.stats)
        assert got.stats["rows_in"] == B[0].size and got.stats["n_keys"] == np.unique(B[0]).size
        for k in np.unique(got["key_id"]).tolist():
            first_rows.setdefault(k, b)
    assert first_rows == {0: 1, 1: 0, 2: 0, 3: 2, 4: 0}, first_rows      # key 0 (2 -> 3 points) first emits in batch 1, key 5 never
    st.close()
    twin.close()


def test_stream_plain_rows_and_parameters(engine):
    """without emit_all a batch emits only its anomalous points, with parameters that change from batch to batch; and the window call
    on the state agrees with the batch about the batch's points"""
    bs, K = batches(tweaks={2: outlier_at(599, 604, 609, 669), 1: outlier_at(100, 128, 135, 143)})     # the last point of every batch
    st = new_state(engine, K, SER | TIMES)
    params = [(0.0, 0), (2.0, 0), (0.0, 129), (1.5, 2)]
    for b, B in enumerate(bs):
        nsigma, ms = params[b]
        got = engine.drop_stream(st, *B, agg_flow="svc", value_op="sum", nsigma=nsigma, min_samples=ms)
        Wb = concat(bs[:b + 1])
        want, no_result = drop_oracle_rows(Wb, nsigma=nsigma or 3.0, ms=ms or 3, judged=Wb[1] >= B[1].min())
        assert_rows(rows_of(got), want, ("plain", b))
        assert got.stats["keys_no_result"] == no_result and got.stats["n_anomalies"] == got.n_rows
        assert 0 < got.n_rows < B[0].size, (b, got.n_rows)
        allrows = rows_of(engine.drop_state(st, nsigma=nsigma, min_samples=ms))
        new = allrows["flow_end_s"] >= B[1].min()
        assert_rows(rows_of(got), {f: allrows[f][new] for f in ROW_FIELDS}, ("plain vs drop_state", b))
    st.close()


# ---- 7. after merge, trim and compact ----
def test_after_merge_trim_and_compact(engine):
    vals = draw_keys([300, 0, 40, 700, 0, 9])
    K = len(vals)
    W = table(vals, [10, 0, 10, 10, 0, 10])
    st = new_state(engine, K, HIST | SER | TIMES)
    keep = W[1] != T_BASE + DAY * 20                         # day 20 arrives late
    fill(engine, st, tuple(c[keep] for c in W))
    engine.merge_stream(st, *(c[~keep] for c in W), agg_flow="svc", value_op="sum")
    got = check_state(engine, st, K, what="merged")
    assert np.array_equal(window(st)[1], W[1]) and got.n_rows == sum(v.size for v in vals)
    assert st.trim(keep_points=520) == 180
    check_state(engine, st, K, what="trimmed")
    remap, cs = st.compact()
    assert st.num_keys == 4 and cs["keys_unseen"] == 2
    check_state(engine, st, 4, what="compacted")
    st.close()


# ---- 8. refusals ----
def test_refusals(engine):
    vals = draw_keys([12, 30])
    W = table(vals)
    nxt = (np.array([0, 1], np.uint64), np.array([T_BASE + DAY * 40] * 2, np.int64), np.array([1 << 50, 1 << 51], np.uint64))
    kw = dict(agg_flow="svc", value_op="sum")
    lib = engine._lib

    def refused(fn, st, what):
        snap = snapshot(st)
        with pytest.raises(TadError) as ei:
            fn()
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT, (what, ei.value)
        assert_same(snapshot(st), snap, what)

    import ctypes as C
    full = new_state(engine, 2, SER | TIMES)
    fill(engine, full, W)
    for flags in (0, HIST, SER):                             # drop_state: plain, history-only, series without times
        st = new_state(engine, 2, flags)
        fill(engine, st, W)
        refused(lambda: engine.drop_state(st), st, ("drop_state flags", flags))
        if not flags & SER:                                  # drop_stream: plain, history-only
            refused(lambda: engine.drop_stream(st, *nxt, **kw), st, ("drop_stream flags", flags))
        st.close()

    def raw(call, st, **fields):
        job = _capi.Job(algo=fields.pop("algo", 3), agg_flow=2, value_op=2, **fields)
        res = C.POINTER(_capi.Result)()
        if call == "state":
            return lib.tad_drop_state(engine._h, st._h, C.byref(job), 0, 0, 0, 0, C.byref(res))
        cols = _capi.Columns(n_rows=2, key_id=nxt[0].ctypes.data, flow_end_s=nxt[1].ctypes.data, value=nxt[2].ctypes.data, num_keys=2, memory=0)
        return lib.tad_drop_stream(engine._h, st._h, C.byref(job), C.byref(cols), 0, C.byref(res))

    snap = snapshot(full)
    for algo in (0, 1, 2):                                   # the algorithm must be DROP
        assert raw("state", full, algo=algo) == -1 and raw("stream", full, algo=algo) == -1
    for bad in (dict(start_time=5), dict(end_time=5), dict(flags=2), dict(flags=4), dict(drop_nsigma=-1.0), dict(drop_min_samples=-1)):
        assert raw("state", full, **bad) == -1, bad
    for bad in (dict(drop_nsigma=-1.0), dict(drop_min_samples=-1), dict(ewma_alpha=1.5)):
        assert raw("stream", full, **bad) == -1, bad
    assert_same(snapshot(full), snap, "raw refusals")
    refused(lambda: engine.drop_state(full, T_BASE + 9, T_BASE + 5), full, "from_t > to_t")
    refused(lambda: engine.drop_stream(full, *nxt, num_keys=3, **kw), full, "num_keys mismatch")
    # the old entry points keep refusing DROP
    refused(lambda: engine.run_state(full, algo="DROP"), full, "run_state")
    refused(lambda: engine.run_state_window(full, T_BASE, 0, 0, algo="DROP"), full, "run_state_window")
    refused(lambda: engine.run_stream(full, *nxt, algo="DROP", **kw), full, "run_stream")
    # stale times: the series imported without its times
    ln, v = full.export_series()
    stale = new_state(engine, 2, SER | TIMES)
    stale.load(full.export())
    stale.load_series(ln, v)
    with pytest.raises(TadError) as ei:
        engine.drop_state(stale)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "times" in ei.value.message
    with pytest.raises(TadError):
        engine.drop_stream(stale, *nxt, **kw)
    stale.close()
    # and after all that the state still takes a batch
    got = engine.drop_stream(full, *nxt, emit_all=True, **kw)
    assert got.n_rows == 2
    full.close()


# ---- 9. the periodical job of theia_amd.drop_detection ----
def test_periodical_drop_detection(engine):
    """feeds of new days give, for those days, the rows of an initial job over everything fed so far; window() the rows of an initial
    job over the days of the range"""
    from theia_amd.drop_detection import RESULT_COLUMNS, PeriodicalDropDetection, drop_detection_table
    parts = [("10.0.0.1", "ingress", 40), ("10.0.0.1", "egress", 2), ("pod-b", "ingress", 17)]
    vals = draw_keys([n for _, _, n in parts], tweaks={0: outlier_at(12, 33), 2: outlier_at(15)})
    ep = np.concatenate([[p[0]] * p[2] for p in parts])
    di = np.concatenate([[p[1]] * p[2] for p in parts])
    day = np.concatenate([19000 + np.arange(p[2]) for p in parts])
    val = np.concatenate(vals)
    pdd = PeriodicalDropDetection(engine)
    cut = 19014
    strip = lambda rows: sorted((r[0],) + r[3:] for r in rows)         # without the fresh ids and the creation time
    for lo, hi in ((0, cut), (cut, 1 << 40)):
        m = (day >= lo) & (day < hi)
        got = pdd.feed(ep[m], di[m], day[m], val[m], detection_id="d1")
        seen = day < hi
        want = [r for r in drop_detection_table(ep[seen], di[seen], day[seen], val[seen], job_type="periodical", engine=engine) if r[7] >= lo]
        assert strip(got) == strip(want) and all(len(r) == len(RESULT_COLUMNS) and r[0] == "periodical" and r[1] == "d1" for r in got)
    assert [r[7] for r in got] == [19033, 19015]                       # (partition, date) order; day 19012's row came with the first feed
    assert pdd.state.num_keys == 3
    win = pdd.window(19005, 19030)
    m = (day >= 19005) & (day < 19030)
    assert strip(win) == strip(drop_detection_table(ep[m], di[m], day[m], val[m], job_type="periodical", engine=engine)) and len(win) >= 1
    with pytest.raises(TadError):                                      # a day that is not newer: the feed fails as a whole
        pdd.feed(["pod-b"], ["ingress"], [19001], [5])
    assert strip(pdd.window()) == strip(drop_detection_table(ep, di, day, val, job_type="periodical", engine=engine))
