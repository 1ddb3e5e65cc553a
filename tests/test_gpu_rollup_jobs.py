"""GPU: what a rolled-up state (tad_state_rollup, include/tad.h) answers and takes afterwards.  The read-only jobs on it return what the
host model (tests/rollup_model.py) says over its folded table; tad_run_state_buckets at the roll-up's bucket and at a multiple of it
returns, on the rolled state, the rows it returns on a twin that never rolled up — bit for bit, over the whole state and over a window
whose bounds are bucket starts; late rows merged into the rolled region, a trim, a compaction and an export / import all keep the state
equal to the model's.  No tolerance in this file."""
import numpy as np
import pytest

from rollup_model import HIST, SER, TIMES, I64, U64
from state_drivers import build, restart, roll
from state_helpers import T_BASE, assert_rows, assert_same, key_values, rows_of, snapshot

pytestmark = pytest.mark.gpu

B_S = 60
T0 = (T_BASE // 3600) * 3600


def table(seed, K=12, span=5400, density=0.25, short=()):
    """K keys with points at seeded seconds of [T0, T0 + span); the keys of `short`: a handful of points each (ARIMA's series)"""
    rng = np.random.default_rng(seed)
    ks, ts, vs = [], [], []
    for key in range(K):
        tk = T0 + np.flatnonzero(rng.random(span) < (0.004 if key in short else density))
        ks.append(np.full(tk.size, key, I64)), ts.append(tk), vs.append(key_values(tk.size, key, rng))
    return K, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs)


@pytest.fixture(scope="module")
def pair(engine):
    """a rolled state (everything older than T0 + 4000 at 60 s), its model, and a twin that never rolled up"""
    cols = table(41)
    rolled, m = build(engine, *cols)
    raw, m_raw = build(engine, *cols)
    got = roll(rolled, m, T0 + 4000, B_S, what="the pair")
    assert got["before_t"] == T0 + 3960 and got["points_after"] * 3 < got["points_before"]
    yield rolled, m, raw, m_raw
    rolled.close(), raw.close()


@pytest.mark.parametrize("algo,params", [("EWMA", {}), ("EWMA", {"alpha": 0.05}), ("DBSCAN", {}), ("DBSCAN", {"eps": 5e7, "min_samples": 3})])
def test_run_state_on_a_rolled_state_is_the_job_over_the_folded_table(engine, pair, algo, params):
    rolled, m, _, _ = pair
    snap = snapshot(rolled)
    n_rows = {}
    for emit_all in (True, False):
        res = engine.run_state(rolled, algo=algo, emit_all=emit_all, **params)
        rows, counters = m.job(algo, emit_all=emit_all, **params)
        assert_rows(rows_of(res), rows, (algo, params, emit_all))
        for f, v in counters.items():
            assert res.stats[f] == v, (algo, f, res.stats[f], v)
        n_rows[emit_all] = res.n_rows
    assert n_rows[False] <= n_rows[True] == m.key.size
    assert_same(snapshot(rolled), snap, "read-only")


def test_arima_on_short_rolled_series(engine):
    cols = table(43, K=6, span=3000, short=range(6))
    st, m = build(engine, *cols, history=False)
    roll(st, m, T0 + 1500, 300, what="arima")
    n, _ = m.per_key()
    assert 4 <= n.max() <= 40
    for emit_all in (True, False):
        res = engine.run_state(st, algo="ARIMA", emit_all=emit_all)
        rows, counters = m.job("ARIMA", emit_all=emit_all)
        assert_rows(rows_of(res), rows, ("ARIMA", emit_all))
        for f, v in counters.items():
            assert res.stats[f] == v, ("ARIMA", f, res.stats[f], v)
    st.close()


@pytest.mark.parametrize("mult", [1, 5])
@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN"])
def test_bucketed_jobs_at_multiples_of_the_bucket_equal_the_unrolled_twins(engine, pair, mult, algo):
    rolled, m, raw, m_raw = pair
    assert m.key.size < m_raw.key.size
    s = B_S * mult
    aligned = (T0 + 600) // s * s, (T0 + 4800) // s * s           # across the bound; both ends bucket starts of the call
    assert aligned[0] < T0 + 3960 < aligned[1]
    some = 0
    for win in ((0, 0), aligned, (aligned[0], 0), (0, aligned[1])):
        for emit_all in (True, False):
            a = engine.run_state_buckets(rolled, s, 0, "sum", *win, algo=algo, emit_all=emit_all)
            b = engine.run_state_buckets(raw, s, 0, "sum", *win, algo=algo, emit_all=emit_all)
            assert_rows(rows_of(a), rows_of(b), (mult, algo, win, emit_all))
            for f in ("n_points", "n_keys", "n_anomalies", "t0"):
                assert a.stats[f] == b.stats[f], (mult, algo, win, f)
            assert a.stats["rows_in"] < b.stats["rows_in"]
            some += a.n_rows
    assert some > 0
    # a bucket that is no multiple of the roll-up's: the rolled state cannot answer it (the header's condition is needed)
    a = engine.run_state_buckets(rolled, 90, 0, "sum", algo=algo, emit_all=True)
    b = engine.run_state_buckets(raw, 90, 0, "sum", algo=algo, emit_all=True)
    assert not np.array_equal(np.asarray(a["throughput"]), np.asarray(b["throughput"]))


def test_late_rows_merged_into_the_rolled_region_then_a_second_roll_up(engine):
    cols = table(47, K=9, span=3000)
    st, m = build(engine, *cols)
    roll(st, m, T0 + 2400, B_S, what="first")
    rng = np.random.default_rng(48)
    k = rng.integers(0, 9, 400).astype(U64)
    t = (T0 + rng.integers(0, 3000, 400)).astype(I64)            # most of them below the bound, beside the buckets' points and on them
    t[:40] = T0 + (rng.integers(0, 40, 40) * B_S)                 # ... and some exactly at bucket starts: they combine
    v = rng.integers(1, 1 << 30, 400).astype(U64)
    stats = engine.merge_stream(st, k, t, v, value_op="sum")
    want = m.merge(k, t, v)
    for f in ("points_inserted", "points_combined", "points_appended"):
        assert stats[f] == want[f], (f, stats[f], want[f])
    assert want["points_combined"] > 0 and want["points_inserted"] > 0
    assert_same(snapshot(st), m.expected_snapshot(), "after the merge")
    assert ((m.t[m.t < T0 + 2400] % B_S) != 0).any()             # late seconds sit beside the buckets' points
    got = roll(st, m, T0 + 2400, B_S, what="second")
    assert got["keys_changed"] > 0 and ((m.t[m.t < T0 + 2400] % B_S) == 0).all()
    st.close()


def test_trim_compact_and_export_import_after_a_roll_up(engine):
    cols = table(51, K=10, span=4000)
    K, k, t, v = cols
    keep = ~np.isin(k, (3, 7))                                   # two unseen keys for the compaction
    late = (k == 5) & (t >= T0 + 900)                            # key 5 ends early: idle for the compaction's time rule
    sel = keep & ~late
    st, m = build(engine, K, k[sel], t[sel], v[sel])
    roll(st, m, T0 + 3000, B_S, what="rolled")
    # a trim that cuts inside the rolled region, on and off a bucket start
    for keep_from in (T0 + 600, T0 + 1230):
        assert st.trim(0, keep_from) == m.trim(0, keep_from) > 0
        assert_same(snapshot(st), m.expected_snapshot(), ("trim", keep_from))
    assert st.trim(40, 0) == m.trim(40, 0) > 0
    assert_same(snapshot(st), m.expected_snapshot(), "trim by count")
    # export / import: a restart
    st = restart(engine, st, HIST | SER | TIMES)
    assert_same(snapshot(st), m.expected_snapshot(), "restart")
    roll(st, m, T0 + 3600, B_S, what="rolled further after the restart")
    # compaction
    remap, stats = st.compact(T0 + 2000)
    want = m.compact(T0 + 2000)
    assert np.array_equal(remap, want["remap"]) and stats["keys_after"] == want["keys_after"] == K - 3
    assert_same(snapshot(st), m.expected_snapshot(), "compact")
    roll(st, m, T0 + 3900, 300, what="a coarser tier after the compaction")
    st.close()
