"""GPU: tad_state_rollup (include/tad.h) — a state's points below a bound folded into time buckets, in place.  The reference is the host
model (tests/rollup_model.py: numpy's floor division and the oracle's Stage 0, then the stream oracle on a fresh state): after every call
the WHOLE export — moments, series, times, history — and the call's counters equal the model's, as bit patterns; no tolerance in this
file.  Every successful call is made twice and the second must change no bit.  The shapes sit on the seams of the kernels: the 64-point
slice and the 2048-point chunk (kHistChunk) of k_win_bucket_fold, the chunk that holds the split, the chunks copied whole behind it."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadEngine, TadError, _capi

from rollup_model import SER, TIMES, I64, U64, RollupModel
from state_drivers import build, roll
from state_helpers import EDGE_RUNS, EDGE_S, EDGE_T0, HIST_CHUNK, T_BASE, assert_same, bits, key_values, new_state, run_times, snapshot, wide_values

pytestmark = pytest.mark.gpu

INV = _capi.TAD_ERR_INVALID_ARGUMENT


# ---- helpers ----


LENS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 4097)
SPLITS = (0, 1, 63, 64, 2047, 2048, 2049, "len-1", "len")
SEAM_S, SEAM_O = 16, 5
SEAM_B = (T_BASE // SEAM_S) * SEAM_S + SEAM_O          # a bucket start: the bound of the seam cases


def seam_keys():
    """one key per (length, split index): `length` consecutive seconds with the point of index `split` at the bound"""
    out = []
    for n in LENS:
        for s in SPLITS:
            s = {"len-1": n - 1, "len": n}.get(s, s)
            if 0 <= s <= n and (n, s) not in out:
                out.append((n, s))
    return out


@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("history", [True, False])
def test_segment_lengths_and_split_indices_on_the_slice_and_chunk_seams(engine, op, history):
    shape = seam_keys()
    assert {n for n, _ in shape} == set(LENS) and len(shape) == 56
    for n in (2049, 4096, 4097):
        assert {s for m_, s in shape if m_ == n} >= {0, 1, 63, 64, 2047, 2048, 2049, n - 1, n}
    rng = np.random.default_rng(5)
    ks, ts, vs = [], [], []
    for key, (n, s) in enumerate(shape):
        ks.append(np.full(n, key, I64)), ts.append(SEAM_B - s + np.arange(n, dtype=I64)), vs.append(wide_values(n, rng, top=0.33))
    st, m = build(engine, len(shape), np.concatenate(ks), np.concatenate(ts), np.concatenate(vs), op=op, history=history)
    k, t, v = m.points()
    assert ((t < SEAM_B).sum(), (t >= SEAM_B).sum()) == (sum(s for _, s in shape), sum(n - s for n, s in shape))
    if op == "sum":                                             # sums of sixteen values of up to 64 bits wrap
        assert any(int(v[i:i + 16].astype(object).sum()) >> 64 for i in range(0, 4096, 16))
    got = roll(st, m, SEAM_B + 3, SEAM_S, SEAM_O, what=("seams", op, history))          # not on a bucket start: floored to SEAM_B
    assert got["before_t"] == SEAM_B and got["points_after"] < got["points_before"]
    n_after, last = m.per_key()
    for key, (n, s) in enumerate(shape):                        # the model, restated per key: ceil(s / 16) buckets and the n - s points kept
        first_bucket = (SEAM_B - s - SEAM_O) // SEAM_S
        assert n_after[key] == (n - s) + ((SEAM_B - 1 - SEAM_O) // SEAM_S - first_bucket + 1 if s else 0), (key, n, s)
    st.close()


@pytest.mark.parametrize("op", ["sum", "max"])
def test_runs_over_several_chunks_and_on_chunk_edges(engine, op):
    """the edge runs of tests/test_gpu_state_buckets.py — a bucket of 4097 and one of 6145 points (three and four chunks), a run that ends
    on a chunk's last point and one that starts on a chunk's first — rolled whole, and rolled up to the start of bucket 3"""
    rng = np.random.default_rng(11)
    ks, ts, vs = [], [], []
    for key, runs in enumerate(EDGE_RUNS):
        tk = run_times(runs, EDGE_S, EDGE_T0, skip=(2,))
        ks.append(np.full(tk.size, key, I64)), ts.append(tk), vs.append(wide_values(tk.size, rng, top=0.33))
    cols = np.concatenate(ks), np.concatenate(ts), np.concatenate(vs)
    assert max(max(r, default=0) for r in EDGE_RUNS) == 6145 > 3 * HIST_CHUNK
    assert EDGE_RUNS[2][:2] == [3, 2045] and EDGE_RUNS[5] == [2048, 2048, 7]            # ends on element 2047; aligned whole chunks
    for before, name in ((EDGE_T0 + 3 * EDGE_S, "to bucket 3"), (EDGE_T0 + 100 * EDGE_S, "whole")):
        st, m = build(engine, len(EDGE_RUNS), *cols, op=op)
        got = roll(st, m, before, EDGE_S, 0, what=("edges", op, name))
        if name == "whole":
            assert got["points_after"] == got["buckets"] == sum(len(r) for r in EDGE_RUNS)
            assert got["keys_changed"] == sum(any(n > 1 for n in r) for r in EDGE_RUNS)
        st.close()


def two_alpha_snapshot(m_built, lost, m_rolled):
    """a state built with one alpha and rolled with another: the keys that lost a point are replayed with the roll-up's alpha over their new
    series, the others keep their moments (n, avg, m2 are the same either way; ewma is the built one's) — last_t is the new series' for all"""
    exp = {p: q for p, q in m_rolled.expected_snapshot().items()}
    state = {f: a.copy() for f, a in exp["state"].items()}
    keep = ~lost
    state["ewma"][keep] = m_built["state"]["ewma"][keep]
    exp["state"] = state
    return exp


def test_points_alone_in_their_bucket_move_in_time_and_keep_their_moments(engine):
    """built with alpha 0.3, rolled with 0.05.  Keys 0..9: one point per bucket, none on a bucket start (times move, nothing folds: the
    moments keep their bits, ewma with 0.3 included; last_t moves for the keys wholly below the bound).  Keys 10..19: three points per
    bucket (replayed with 0.05)"""
    B_S, O = 60, 7
    b = (T_BASE // B_S) * B_S + O
    rng = np.random.default_rng(9)
    ks, ts, vs = [], [], []
    for key in range(20):
        n = 30 + key
        j = np.arange(n, dtype=I64) - (n if key % 2 else 20)     # odd keys wholly below the bound, even keys across it
        tk = b + j * B_S + 1 + (key % 50)
        if key >= 10:
            tk = np.sort(np.concatenate([tk, tk + 3, tk + 5]))
        ks.append(np.full(tk.size, key, I64)), ts.append(tk), vs.append(key_values(tk.size, key, rng))
    st, m = build(engine, 20, np.concatenate(ks), np.concatenate(ts), np.concatenate(vs), op="sum", alpha=0.3)
    built = m.expected_snapshot()
    lost = m.lost_a_point(b, B_S, O)
    assert lost.tolist() == [False] * 10 + [True] * 10
    m2 = RollupModel(20, m.flags, "sum", 0.05)
    m2._set(*m.points())
    got = roll(st, m2, b, B_S, O, alpha=0.05, what="alone", expected=lambda: two_alpha_snapshot(built, lost, m2))
    assert got["keys_changed"] == 10 and got["points_rolled"] > got["buckets"]
    after = st.export()
    for f in ("n", "avg", "m2", "ewma"):
        assert np.array_equal(bits(after[f][:10]), bits(built["state"][f][:10])), f
    assert not np.array_equal(bits(after["ewma"][10:]), bits(built["state"]["ewma"][10:]))
    moved = after["last_t"] != built["state"]["last_t"]
    assert moved.tolist() == [bool(key % 2) for key in range(20)]
    assert ((after["last_t"][moved] - O) % B_S == 0).all()
    st.close()


def test_last_t_moves_and_the_next_stream_batch_is_judged_against_it(engine):
    B_S = 100
    b0 = (T_BASE // B_S) * B_S
    # key 0 wholly below the bound, its newest point 40 s into its last bucket; key 1 wholly at or after it; key 2 across; key 3 unseen
    k = np.array([0, 0, 0, 1, 1, 2, 2, 2])
    t = np.array([b0 + 10, b0 + 20, b0 + 140, b0 + 300, b0 + 301, b0 + 50, b0 + 299, b0 + 300])
    v = np.arange(1, 9) * 1000
    st, m = build(engine, 4, k, t, v)
    before = st.export()["last_t"].copy()
    got = roll(st, m, b0 + 300, B_S, what="last_t")
    assert got["keys_changed"] == 1 and got["points_rolled"] == 5 and got["buckets"] == 4
    last = st.export()["last_t"]
    assert last.tolist() == [b0 + 100, b0 + 301, b0 + 300, 0] and before.tolist() == [b0 + 140, b0 + 301, b0 + 300, 0]
    snap = snapshot(st)
    one = lambda tt: (np.array([0], U64), np.array([tt], I64), np.array([777], U64))
    with pytest.raises(TadError):
        engine.run_stream(st, *one(b0 + 100), value_op="sum")                         # the bucket's start: not newer than last_t
    assert_same(snapshot(st), snap, "a refused batch")
    engine.run_stream(st, *one(b0 + 120), value_op="sum")                             # inside the last bucket, before the old newest point
    m.append(*one(b0 + 120))
    assert_same(snapshot(st), m.expected_snapshot(), "after the accepted batch")
    roll(st, m, b0 + 300, B_S, what="the batch's point folded by a later roll-up")
    assert m.t[m.key == 0].tolist() == [b0, b0 + 100] and m.value[m.key == 0].tolist() == [3000, 3777]
    st.close()


@pytest.mark.parametrize("op", ["sum", "max"])
def test_negative_times_a_non_zero_origin_and_a_bound_off_the_bucket_start(engine, op):
    rng = np.random.default_rng(21)
    K = 40
    ks, ts = [], []
    for key in range(K):
        tk = -6000 + np.flatnonzero(rng.random(12000) < 0.02 * (1 + key % 5))
        ks.append(np.full(tk.size, key, I64)), ts.append(tk)
    k, t = np.concatenate(ks), np.concatenate(ts).astype(I64)
    st, m = build(engine, K, k, t, wide_values(k.size, rng, top=0.2), op=op)
    raw = tuple(a.copy() for a in m.points())
    got = roll(st, m, -100, 600, 250, what=("negative", op))
    assert got["before_t"] == -350
    inside = (raw[1] >= -350) & (raw[1] < -100)
    assert inside.any() and np.isin(raw[1][inside], m.t).all()                       # the points in [b, before_t) stay
    got = roll(st, m, 3001, 7, 3, what=("negative, a second tier", op))
    assert got["before_t"] == 2999 and (got["before_t"] - 3) % 7 == 0
    st.close()


@pytest.mark.parametrize("K,history,ties", [(40, True, True), (40, False, False), (9000, True, False)])
def test_key_counts_below_and_above_8192_ties_and_the_history(engine, K, history, ties):
    rng = np.random.default_rng(K)
    n = 1 + (np.arange(K) * 7 + 3) % (200 if K == 40 else 24)
    n[::17] = 0                                                                       # unseen keys among them
    ks = np.repeat(np.arange(K), n)
    ts = np.concatenate([T_BASE + np.sort(rng.choice(3600, size=c, replace=False)) for c in n]).astype(I64)
    vs = np.concatenate([key_values(c, key, rng, ties=ties) for key, c in enumerate(n)]) if ks.size else np.zeros(0)
    st, m = build(engine, K, ks, ts, vs, history=history)
    got = roll(st, m, T_BASE + 3000, 300, 11, what=("keys", K))
    assert 0 < got["keys_changed"] < K and got["points_after"] < got["points_before"]
    if ties:
        h = st.export_history()[1]
        assert np.unique(h).size < h.size
    roll(st, m, T_BASE + 4000, 3600, 311, what=("keys, coarser and further", K))
    st.close()


def day_state(engine, seed=31, K=6, span=20000):
    rng = np.random.default_rng(seed)
    t0 = (T_BASE // 3600) * 3600
    ks, ts = [], []
    for key in range(K):
        tk = t0 + np.flatnonzero(rng.random(span) < 0.4)
        ks.append(np.full(tk.size, key, I64)), ts.append(tk)
    k = np.concatenate(ks)
    return t0, (K, k, np.concatenate(ts), wide_values(k.size, rng, top=0.1))


@pytest.mark.parametrize("op", ["sum", "max"])
def test_60_then_3600_is_3600_and_the_tiers_commute(engine, op):
    t0, cols = day_state(engine)
    a, ma = build(engine, *cols, op=op)
    b, mb = build(engine, *cols, op=op)
    bound = t0 + 4 * 3600
    roll(a, ma, bound + 59, 60, what="60"), roll(a, ma, bound, 3600, what="then 3600")
    roll(b, mb, bound, 3600, what="3600")
    assert_same(snapshot(a), snapshot(b), "60 then 3600 against 3600")
    a.close(), b.close()
    a, ma = build(engine, *cols, op=op)
    b, mb = build(engine, *cols, op=op)
    old, recent = t0 + 2 * 3600, t0 + 5 * 3600 - 120
    roll(a, ma, old, 3600, what="old first"), roll(a, ma, recent, 60, what="then recent")
    roll(b, mb, recent, 60, what="recent first"), roll(b, mb, old, 3600, what="then old")
    assert_same(snapshot(a), snapshot(b), "the tiers in both orders")
    a.close(), b.close()


def test_state_bytes_fall(engine):
    t0, cols = day_state(engine, K=8, span=40000)
    st, m = build(engine, *cols)
    before = st.nbytes()
    got = roll(st, m, t0 + 39000, 60, what="bytes")
    assert got["points_after"] * 8 < got["points_before"]
    assert st.nbytes() < before // 2, (st.nbytes(), before)
    st.close()


def test_nothing_below_the_bound_and_an_empty_state(engine):
    st, m = build(engine, 3, [0, 0, 2], [T_BASE + 5, T_BASE + 6, T_BASE + 9], [5, 6, 7])
    snap = snapshot(st)
    got = st.rollup(T_BASE + 5, 5, T_BASE % 5)
    assert got["before_t"] == T_BASE + 5 and (got["points_before"], got["points_after"], got["points_rolled"], got["buckets"], got["keys_changed"]) == (3, 3, 0, 0, 0)
    assert_same(snapshot(st), snap, "nothing below the bound")
    st.close()
    empty = new_state(engine, 5)
    got = empty.rollup(T_BASE, 60)
    assert (got["points_before"], got["points_after"], got["points_rolled"]) == (0, 0, 0) and got["before_t"] == T_BASE // 60 * 60
    assert empty.series_points() == 0 and not empty.export()["n"].any()
    empty.close()


def raw_rollup(engine, st, before, bucket_s, origin, op, alpha):
    return engine._lib.tad_state_rollup(engine._h, st._h, before, bucket_s, origin, op, alpha, None)


def test_every_refusal_leaves_the_export_unchanged(engine):
    st, m = build(engine, 3, [0, 0, 0, 1, 2], T_BASE + np.array([1, 2, 70, 5, 9]), [5, 6, 7, 8, 9])
    snap = snapshot(st)
    SUM, MAX, AUTO = _capi.TAD_OP["sum"], _capi.TAD_OP["max"], _capi.TAD_OP["auto"]
    bad = [(T_BASE + 60, 0, 0, SUM, 0.0), (T_BASE + 60, -5, 0, SUM, 0.0), (T_BASE + 60, 60, 60, SUM, 0.0), (T_BASE + 60, 60, -1, SUM, 0.0),
           (T_BASE + 60, 60, 0, AUTO, 0.0), (T_BASE + 60, 60, 0, 7, 0.0), (T_BASE + 60, 60, 0, MAX, -0.1), (T_BASE + 60, 60, 0, MAX, 1.5),
           (T_BASE + 60, 60, 0, SUM, float("nan")), (1 << 62, 60, 0, SUM, 0.0), (-(1 << 62), 60, 0, SUM, 0.0)]
    for args in bad:
        assert raw_rollup(engine, st, *args) == INV, args
        assert_same(snapshot(st), snap, args)
    rs = _capi.RollupStats(points_before=99)
    assert engine._lib.tad_state_rollup(engine._h, None, T_BASE, 60, 0, SUM, 0.0, C.byref(rs)) == INV and rs.points_before == 0
    with pytest.raises(ValueError):
        st.rollup(T_BASE + 60, 60, op="auto")
    # what the state must keep
    for kw in (dict(), dict(history=True), dict(series=True), dict(history=True, series=True)):
        other = engine.state_create(3, **kw)
        with pytest.raises(TadError) as ei:
            other.rollup(T_BASE, 60)
        assert ei.value.code == INV and "TAD_STATE_SERIES | TAD_STATE_TIMES" in str(ei.value)
        other.close()
    # stale times: a series imported without its times
    stale = new_state(engine, 3)
    stale.load(snap["state"]), stale.load_history(*snap["history"]), stale.load_series(*snap["series"])
    with pytest.raises(TadError) as ei:
        stale.rollup(T_BASE + 60, 60)
    assert ei.value.code == INV and "tad_state_import_times" in str(ei.value)
    stale.load_times(snap["times"])
    assert stale.rollup(T_BASE + 60, 60)["keys_changed"] == 1                         # the good call, after all of them
    st.rollup(T_BASE + 60, 60)
    assert_same(snapshot(stale), snapshot(st), "the good call")
    m.rollup(T_BASE + 60, 60)
    assert_same(snapshot(st), m.expected_snapshot(), "the good call against the model")
    stale.close(), st.close()


def test_a_workspace_limit_too_small_refuses_and_leaves_the_export_unchanged(engine):
    """60000 keys need about 2.5 MB of per-key and per-chunk scratch: over a limit of 1 MiB.  The state is built on the session's engine
    and imported (an import needs no workspace)"""
    K = 60000
    k = np.repeat(np.arange(K), 2)
    t = np.tile(np.array([T_BASE + 1, T_BASE + 2], I64), K)
    big, m = build(engine, K, k, t, np.arange(2 * K) + 1000, history=False)
    snap = snapshot(big)
    big.close()
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    st = new_state(small, K, SER | TIMES)
    st.load(snap["state"]), st.load_series(*snap["series"]), st.load_times(snap["times"])
    with pytest.raises(TadError) as ei:
        st.rollup(T_BASE + 60, 60)
    assert ei.value.code == _capi.TAD_ERR_GRID_TOO_LARGE and "workspace limit" in str(ei.value)
    assert_same(snapshot(st), snap, "refused by the workspace limit")
    st.close(), small.close()
