"""GPU: streaming DBSCAN (tad_run_stream with TAD_ALGO_DBSCAN on a state with history, include/tad.h).  The defining property: the rows
of batch b are exactly the rows tad_run(DBSCAN) emits, over batches 1..b concatenated with the same job parameters, for the points of
batch b — key, time, throughput, algo_calc and stddev bit for bit, in the same order (emit_all: all of batch b's points with their
verdicts).  Float columns are compared as uint64 bit patterns.  The history holds n[k] values per key after every batch, and a failed
batch leaves state and history as they were."""
import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadEngine, TadError
from state_helpers import SKIP, STATE_FIELDS, T_BASE, assert_rows, assert_same, bits, minute_batches, point_codes, restrict, rows_of, snapshot

pytestmark = pytest.mark.gpu


def batch_job_rows(engine, K, batches, upto, op, emit_all=False, eps=0.0, min_samples=0, pod=False):
    """tad_run(DBSCAN) over batches[0..upto] concatenated, restricted to batch `upto`'s points"""
    cat = [np.concatenate([b[i] for b in batches[:upto + 1]]) for i in range(len(batches[0]))]
    kw = dict(key_id2=cat[3]) if pod else {}
    res = engine.run("DBSCAN", cat[0], cat[1], cat[2], K, agg_flow="pod" if pod else "svc", value_op=op, emit_all=emit_all, eps=eps, min_samples=min_samples, **kw)
    b = batches[upto]
    return restrict(rows_of(res), point_codes(b[0], b[1], b[3] if pod else None))


def oracle_rows(K, batches, upto, op, eps, min_samples, emit_all=False):
    """the same from tad_oracle: Stage 0 of the concatenated table, dbscan_noise_1d per key, batch `upto`'s points"""
    cat = [np.concatenate([b[i] for b in batches[:upto + 1]]) for i in range(3)]
    pk, pt, pv = orc.stage0(cat[0], cat[1], cat[2], op)
    keys, ptr = orc.series_offsets(pk)
    noise = np.zeros(pk.size, bool)
    x = orc.u64_to_f64(pv)
    for i in range(keys.size):
        noise[ptr[i]:ptr[i + 1]] = orc.dbscan_noise_1d(x[ptr[i]:ptr[i + 1]], eps, min_samples)
    b = batches[upto]
    mine = np.isin((pk << np.uint64(32)) | (pt - T_BASE + (1 << 31)).astype(np.uint64), point_codes(b[0], b[1]))
    sel = mine & (noise | emit_all)
    return pk[sel], pt[sel], x[sel], noise[sel]


def assert_history(st):
    n = st.export()["n"]
    ln, vals = st.export_history()
    assert st.history_points() == int(n.sum()) == vals.size
    assert np.array_equal(ln, n.astype(np.uint64))
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    for k in np.flatnonzero(ln > 1)[:2000]:
        assert (vals[off[k]:off[k + 1] - 1] <= vals[off[k] + 1:off[k + 1]]).all(), k


def second_batches(K, pts_per_key, rows_per_point, seed, span, width):
    rng = np.random.default_rng(seed)
    pts = np.broadcast_to(np.asarray(pts_per_key, dtype=np.int64), (K,))
    pk = np.repeat(np.arange(K, dtype=np.uint64), pts)
    pt = T_BASE + rng.integers(0, span, size=pk.size).astype(np.int64)
    base = 1_000_000_000 + (orc.mix64(pk + np.uint64(5)) % np.uint64(3_000_000_000)).astype(np.int64)
    k, t = np.repeat(pk, rows_per_point), np.repeat(pt, rows_per_point)
    v = (np.repeat(base, rows_per_point) + rng.integers(-3_000_000, 3_000_000, size=k.size)).astype(np.uint64)
    v = np.where(rng.random(k.size) < 5e-3, v * np.uint64(3), v)
    order = rng.permutation(k.size)
    k, t, v = k[order], t[order], v[order]
    b = (t - T_BASE) // width
    return [(k[b == h], t[b == h], v[b == h]) for h in range(int(b.max()) + 1)]


# ---- 1. convergence to the batch job ----
@pytest.mark.parametrize("n_rows,K,T,cuts", [(60000, 200, 120, (40, 80)), (3000, 7, 64, (1, 2, 3, 60))])
@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("emit_all", [False, True])
@pytest.mark.parametrize("eps", [0.0, 3e6])
def test_batches_equal_the_batch_job(engine, n_rows, K, T, cuts, op, emit_all, eps):
    batches = minute_batches(n_rows, K, T, cuts)
    st = engine.state_create(K, history=True)
    noise_seen = 0
    for b, (bk, bt, bv) in enumerate(batches):
        got = engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op=op, algo="DBSCAN", emit_all=emit_all, eps=eps)
        assert_rows(rows_of(got), batch_job_rows(engine, K, batches, b, op, emit_all=emit_all, eps=eps), (b, op, emit_all))
        noise_seen += int(got["anomaly"].sum()) if emit_all else got.n_rows
        assert_history(st)
    assert noise_seen > 0
    st.close()


# ---- 2. exactness beyond the fast path ----
def crafted_batches():
    """per batch (key, t, v): key 0 a chain exactly eps apart, key 1 grows 1, 2, 3, 5 points, key 2 values >= 2^53 (neighbours collapse
    in float64), key 3 two clusters and outliers, key 4 one point"""
    eps = 1024.0
    rng = np.random.default_rng(5)
    out = []
    t = T_BASE
    for b in range(4):
        k, tt, v = [], [], []

        def add(key, vals):
            nonlocal t
            for x in vals:
                k.append(key); tt.append(t); v.append(int(x)); t += 60
        add(0, [10_000_000 + 1024 * (3 * j + b) for j in range(3)])
        add(1, [5_000_000 + 1000 * b] * (1 if b < 3 else 2))
        add(2, [(1 << 60) + int(d) for d in rng.integers(0, 1 << 12, size=4)] + [(1 << 60) + (1 << 20) * (b + 1)])
        add(3, list(7_000_000 + rng.integers(0, 800, size=3)) + list(9_000_000 + rng.integers(0, 800, size=2)) + [int(8e6) + 10_000 * b])
        if b == 0:
            add(4, [123456789])
        out.append((np.array(k, np.uint64), np.array(tt, np.int64), np.array(v, np.uint64)))
    return out, eps


@pytest.mark.parametrize("min_samples", [0, 2, 3])
@pytest.mark.parametrize("emit_all", [False, True])
def test_exact_beyond_the_fast_path(engine, min_samples, emit_all):
    batches, eps = crafted_batches()
    K = 5
    ms = min_samples or 4
    st = engine.state_create(K, history=True)
    for b, (bk, bt, bv) in enumerate(batches):
        got = rows_of(engine.run_stream(st, bk, bt, bv, agg_flow="svc", value_op="sum", algo="DBSCAN", emit_all=emit_all, eps=eps,
                                        min_samples=min_samples))
        assert_rows(got, batch_job_rows(engine, K, batches, b, "sum", emit_all=emit_all, eps=eps, min_samples=min_samples), b)
        ok, ot, ox, on = oracle_rows(K, batches, b, "sum", eps, ms, emit_all)
        assert np.array_equal(got["key_id"], ok) and np.array_equal(got["flow_end_s"], ot) and np.array_equal(bits(got["throughput"]), bits(ox))
        if emit_all:
            assert np.array_equal(got["anomaly"].astype(bool), on)
        n = st.export()["n"]
        if emit_all:   # a key below min_samples points: every point of its batch is noise
            few = got["anomaly"][n[got["key_id"].astype(np.int64)] < ms]
            assert (few == 1).all()
    assert_history(st)
    st.close()


def test_parameters_may_change_between_batches(engine):
    batches = minute_batches(20000, 50, 90, (30, 60))
    st = engine.state_create(50, history=True)
    for b, ((bk, bt, bv), (eps, ms)) in enumerate(zip(batches, ((0.0, 0), (2e6, 3), (5e6, 6)))):
        got = engine.run_stream(st, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=eps, min_samples=ms, emit_all=True)
        assert_rows(rows_of(got), batch_job_rows(engine, 50, batches, b, "auto", emit_all=True, eps=eps, min_samples=ms), b)
    st.close()


# ---- 3. both Stage-0 forms, long keys ----
def test_second_resolution_batches_and_forced_forms(engine):
    K = 3000
    batches = second_batches(K, 20, 3, seed=32, span=6 * 3600, width=3600)
    outs = []
    for plan, paths in (({"sparse": "always", "sparse_sort": "lsd"}, (4,)), ({"sparse": "never"}, (1, 2, 3)),
                        ({"sparse": "always", "sparse_sort": "partition", "stage0": "v2"}, (8,))):
        with engine.plan(**plan):
            st = engine.state_create(K, history=True)
            res = []
            for b, (bk, bt, bv) in enumerate(batches):
                r = engine.run_stream(st, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=2e6, emit_all=True)
                assert r.stats["stage0_path"] in paths, (plan, b, r.stats["stage0_path"])
                res.append(rows_of(r))
            assert_history(st)
            outs.append((res, st.export(), st.export_history()))
            st.close()
    for b in range(len(batches)):
        assert_rows(outs[0][0][b], batch_job_rows(engine, K, batches, b, "sum", emit_all=True, eps=2e6), b)
    for res, state, (ln, vals) in outs[1:]:
        for b in range(len(batches)):
            assert_rows(res[b], outs[0][0][b], b)
        for f in STATE_FIELDS:
            assert np.array_equal(bits(state[f]), bits(outs[0][1][f])), f
        assert np.array_equal(ln, outs[0][2][0]) and np.array_equal(vals, outs[0][2][1])


def test_long_keys(engine):
    """two keys reach >= 20 000 history points, with more points in one batch than the LDS sort holds (global-memory sort) and a
    merge split over many wavefronts; the other keys stay short"""
    rng = np.random.default_rng(77)
    K = 40
    batches = []
    t0 = T_BASE
    for b, n_long in enumerate((12000, 9000, 600)):
        ks, ts, vs = [], [], []
        for key in (0, 1):
            t = t0 + np.arange(n_long, dtype=np.int64)
            v = 2_000_000_000 + rng.integers(0, 40_000_000, size=n_long)
            v[rng.random(n_long) < 0.01] *= 3
            ks.append(np.full(n_long, key, np.uint64)); ts.append(t); vs.append(v.astype(np.uint64))
        kk = rng.integers(2, K, size=500).astype(np.uint64)
        ks.append(kk); ts.append(t0 + rng.integers(0, n_long, size=500).astype(np.int64)); vs.append(rng.integers(1_000_000_000, 1_010_000_000, size=500).astype(np.uint64))
        k, t, v = np.concatenate(ks), np.concatenate(ts), np.concatenate(vs)
        order = rng.permutation(k.size)
        batches.append((k[order], t[order], v[order]))
        t0 += n_long
    for plan in ({"sparse": "always"}, {"sparse": "never"}):
        with engine.plan(**plan):
            st = engine.state_create(K, history=True)
            for b, (bk, bt, bv) in enumerate(batches):
                got = engine.run_stream(st, bk, bt, bv, agg_flow="", value_op="max", algo="DBSCAN", eps=1e5, emit_all=True)
                assert_rows(rows_of(got), batch_job_rows(engine, K, batches, b, "max", emit_all=True, eps=1e5), (plan, b))
            assert (st.export()["n"][:2] >= 20000).all()
            assert_history(st)
            st.close()


# ---- 4. pod mode and narrow columns ----
def test_pod_mode_and_narrow_columns(engine):
    K = 300
    batches = minute_batches(40000, K, 100, (30, 70))
    rng = np.random.default_rng(3)
    batches = [(k, t, v, np.where(rng.random(k.size) < 0.3, SKIP, (k + np.uint64(7)) % np.uint64(K))) for k, t, v in batches]
    st = engine.state_create(K, history=True)
    st32 = engine.state_create(K, history=True)
    for b, (bk, bt, bv, bk2) in enumerate(batches):
        got = rows_of(engine.run_stream(st, bk, bt, bv, key_id2=bk2, agg_flow="pod", algo="DBSCAN", eps=3e6))
        assert_rows(got, batch_job_rows(engine, K, batches, b, "auto", eps=3e6, pod=True), b)
        k32 = np.where(bk2 == SKIP, np.uint32(0xFFFFFFFF), bk2.astype(np.uint32))
        got32 = rows_of(engine.run_stream(st32, bk.astype(np.uint32), bt.astype(np.uint32), bv, key_id2=k32, agg_flow="pod", algo="DBSCAN",
                                          eps=3e6))
        assert_rows(got32, got, b)
    assert_history(st)
    assert np.array_equal(st.export_history()[1], st32.export_history()[1])
    st.close()
    st32.close()


# ---- 5. mixed algos on one history state ----
def test_ewma_batches_on_a_history_state(engine):
    K = 200
    batches = minute_batches(60000, K, 120, (30, 60, 90))
    hist = engine.state_create(K, history=True)
    plain = engine.state_create(K)
    for b, (bk, bt, bv) in enumerate(batches):
        want = engine.run_stream(plain, bk, bt, bv, agg_flow="svc")
        if b % 2 == 0:
            assert_rows(rows_of(engine.run_stream(hist, bk, bt, bv, agg_flow="svc")), rows_of(want), b)
        else:
            got = engine.run_stream(hist, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=3e6)
            assert_rows(rows_of(got), batch_job_rows(engine, K, batches, b, "sum", eps=3e6), b)
        a, p = hist.export(), plain.export()
        for f in STATE_FIELDS:
            assert np.array_equal(bits(a[f]), bits(p[f])), (b, f)
        assert plain.history_points() == 0
        assert_history(hist)
    hist.close()
    plain.close()


# ---- 6. rejections leave everything untouched ----


def test_rejections(engine):
    K = 100
    batches = minute_batches(20000, K, 60, (30,))
    plain = engine.state_create(K)
    engine.run_stream(plain, *batches[0], agg_flow="svc")
    snap = snapshot(plain)
    with pytest.raises(TadError) as ei:
        engine.run_stream(plain, *batches[1], agg_flow="svc", algo="DBSCAN")
    assert ei.value.code == -1
    assert_same(snapshot(plain), snap, "the state changed")
    with pytest.raises(TadError):
        plain.export_history()
    plain.close()

    st = engine.state_create(K, history=True)
    engine.run_stream(st, *batches[0], agg_flow="svc", algo="DBSCAN")
    snap = snapshot(st)
    for algo in ("ARIMA", "DROP"):
        with pytest.raises(TadError) as ei:
            engine.run_stream(st, *batches[1], agg_flow="svc", algo=algo)
        assert ei.value.code == -1
        assert_same(snapshot(st), snap, "the state changed")
    with pytest.raises(TadError) as ei:                                      # a late row (batch 0 again)
        engine.run_stream(st, *batches[0], agg_flow="svc", algo="DBSCAN")
    assert ei.value.code == -1
    assert_same(snapshot(st), snap, "the state changed")
    got = engine.run_stream(st, *batches[1], agg_flow="svc", algo="DBSCAN")   # the state goes on as if nothing had happened
    assert_rows(rows_of(got), batch_job_rows(engine, K, batches, 1, "sum"))
    st.close()


# ---- 7. restart and growth ----
def test_restart_and_growth(engine):
    K = 150
    batches = minute_batches(50000, K, 120, (30, 60, 90))
    ref = engine.state_create(K, history=True)
    for bk, bt, bv in batches[:2]:
        engine.run_stream(ref, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=3e6)
    moments, (ln, vals) = ref.export(), ref.export_history()

    fresh = engine.state_create(K, history=True)
    fresh.load(moments)
    snap = snapshot(fresh)
    bad_len = ln.copy()
    k = int(np.flatnonzero(ln > 0)[0])
    bad_len[k] -= 1
    with pytest.raises(TadError) as ei:
        fresh.load_history(bad_len, vals[:-1])
    assert ei.value.code == -1
    assert_same(snapshot(fresh), snap, "the state changed")
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    k = int(np.flatnonzero([vals[off[i]] != vals[off[i + 1] - 1] if ln[i] > 1 else False for i in range(K)])[0])
    unsorted = vals.copy()
    unsorted[off[k]], unsorted[off[k + 1] - 1] = vals[off[k + 1] - 1], vals[off[k]]
    with pytest.raises(TadError) as ei:
        fresh.load_history(ln, unsorted)
    assert ei.value.code == -1
    assert_same(snapshot(fresh), snap, "the state changed")
    plain = engine.state_create(K)
    plain.load(moments)
    with pytest.raises(TadError) as ei:
        plain.load_history(ln, vals)
    assert ei.value.code == -1
    plain.close()

    fresh.load_history(ln, vals)
    assert fresh.history_points() == vals.size
    for bk, bt, bv in batches[2:]:
        a = engine.run_stream(ref, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=3e6, emit_all=True)
        b = engine.run_stream(fresh, bk, bt, bv, agg_flow="svc", algo="DBSCAN", eps=3e6, emit_all=True)
        assert_rows(rows_of(b), rows_of(a))
    ref.close()

    # growth: the added keys start with empty histories and take part in the next batch
    K2 = K + 60
    fresh.resize(K2)
    ln2, vals2 = fresh.export_history()
    assert ln2.size == K2 and (ln2[K:] == 0).all() and np.array_equal(vals2, fresh.export_history()[1])
    rng = np.random.default_rng(9)
    t_next = int(batches[-1][1].max()) + 60
    nk = rng.integers(0, K2, size=4000).astype(np.uint64)
    nt = t_next + 60 * rng.integers(0, 20, size=nk.size).astype(np.int64)
    nv = (2_000_000_000 + rng.integers(0, 20_000_000, size=nk.size)).astype(np.uint64)
    grown = batches + [(nk, nt, nv)]
    got = engine.run_stream(fresh, nk, nt, nv, agg_flow="svc", algo="DBSCAN", eps=3e6, emit_all=True)
    assert_rows(rows_of(got), batch_job_rows(engine, K2, grown, len(grown) - 1, "sum", emit_all=True, eps=3e6))
    assert (np.asarray(got["key_id"]) >= K).any()
    assert_history(fresh)
    fresh.close()
