"""GPU: a batch placed by time into a streaming state (tad_state_merge, include/tad.h).  The defining property: after a merge the state —
moments, series, times, history — is bit for bit the state a fresh state of the same flags holds after ONE tad_run_stream EWMA batch
over every raw row fed so far.  Two references: (R1) the engine itself, that fresh state; (R2) oracle.stream_oracle.run_stream on a
fresh StreamState plus oracle.tad_oracle.stage0 for series / times / sorted history.  The call's counters (inserted, combined, appended,
replayed) are compared with a host-side set computation, so no case passes on a path that only appends.  Floats are compared as uint64
bit patterns."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import stream_oracle as sorc
from oracle import tad_oracle as orc
from theia_amd import TadError, _capi
from theia_amd.engine import DeviceArray
from state_helpers import (ALL, HIST, SER, STATE_FIELDS, TIMES, T_BASE, U64, assert_counts, assert_rows, assert_same, expected_counts, new_state,
                           rows_of, snapshot)

pytestmark = pytest.mark.gpu


def cat(batches):
    return tuple(np.concatenate([b[i] for b in batches]) for i in range(3))


def r1_snapshot(engine, K, flags, rows, op, alpha=0.0, k2=None):
    """R1: a fresh state, ONE run_stream EWMA batch over all raw rows"""
    st = new_state(engine, K, flags)
    if rows[0].size:
        engine.run_stream(st, rows[0], rows[1], rows[2], value_op=op, alpha=alpha, key_id2=k2)
    snap = snapshot(st)
    st.close()
    return snap


def r2_snapshot(K, flags, rows, op, alpha=0.5):
    """R2: the stream oracle on a fresh state; series / times / history from the oracle's Stage 0"""
    os_ = sorc.StreamState(K)
    pk, pt, pv = orc.stage0(rows[0], rows[1], rows[2], op)
    if pk.size:
        sorc.run_stream(os_, rows[0], rows[1], rows[2], op=op, alpha=alpha)
    ln = np.bincount(pk.astype(np.int64), minlength=K).astype(np.uint64)
    hv = pv[np.lexsort((pv, pk))]
    return {"state": {f: getattr(os_, f) for f in STATE_FIELDS}, "history": (ln, hv) if flags & HIST else None, "series": (ln, pv),
            "times": pt if pk.size else None}


def check_run_state(engine, st, rows, op, algos=("EWMA", "DBSCAN"), emit=(False, True), what="", k2=None):
    """run_state on the merged state == tad_run over the raw rows"""
    for algo in algos:
        for emit_all in emit:
            got = engine.run_state(st, algo=algo, emit_all=emit_all)
            want = engine.run(algo, rows[0], rows[1], rows[2], st.num_keys, value_op=op, emit_all=emit_all, key_id2=k2)
            assert_rows(rows_of(got), rows_of(want), (what, algo, emit_all))


def lagged_batches():
    """case 1's table: every row delayed by 1-3 buckets with probability 0.2, batches by ARRIVAL bucket"""
    k, t, v = orc.synth_rows(0, 60000, 300, 48)
    rng = np.random.default_rng(7)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    arrival = bucket + np.where(rng.random(k.size) < 0.2, rng.integers(1, 4, size=k.size), 0)
    edges = (0, 8, 16, 24, 32, 40, 1 << 30)
    return [(k[(arrival >= lo) & (arrival < hi)], t[(arrival >= lo) & (arrival < hi)], v[(arrival >= lo) & (arrival < hi)])
            for lo, hi in zip(edges[:-1], edges[1:])]


# ---- 1. lagged arrival on the minute lattice ----
@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("flags", [ALL, SER | TIMES], ids=["flags11", "flags10"])
def test_lagged_arrival_minute_lattice(engine, op, flags):
    K = 300
    batches = lagged_batches()
    st = new_state(engine, K, flags)
    for b, batch in enumerate(batches):
        prev, sofar = cat(batches[:b]) if b else (np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64)), cat(batches[:b + 1])
        stats = engine.merge_stream(st, *batch, value_op=op)
        want = expected_counts(prev, batch, op)
        assert_counts(stats, want, b)
        assert stats["rows_in"] == stats["rows_used"] == batch[0].size
        if b:
            for f in ("points_inserted", "points_combined", "points_appended", "keys_replayed"):
                assert stats[f] > 0, (b, f)
        else:
            assert stats["keys_replayed"] == stats["points_inserted"] == stats["points_combined"] == 0
        snap = snapshot(st)
        assert_same(snap, r1_snapshot(engine, K, flags, sofar, op), (b, "R1"))
        assert_same(snap, r2_snapshot(K, flags, sofar, op), (b, "R2"))
        check_run_state(engine, st, sofar, op, algos=("EWMA", "DBSCAN") if flags & HIST else ("EWMA",), what=b)
    check_run_state(engine, st, cat(batches), op, algos=("ARIMA",), emit=(False,), what="end")
    st.close()


# ---- 2. rows in arbitrary order ----
@pytest.mark.parametrize("op", ["sum", "max"])
def test_rows_in_arbitrary_order(engine, op):
    K = 300
    k, t, v = orc.synth_rows(0, 60000, K, 48)
    order = np.random.default_rng(11).permutation(k.size)
    k, t, v = k[order], t[order], v[order]
    batches = [(k[lo:lo + 12000], t[lo:lo + 12000], v[lo:lo + 12000]) for lo in range(0, 60000, 12000)]
    st = new_state(engine, K)
    for b, batch in enumerate(batches):
        stats = engine.merge_stream(st, *batch, value_op=op)
        prev = cat(batches[:b]) if b else (np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64))
        assert_counts(stats, expected_counts(prev, batch, op), b)
        if b:
            assert stats["points_inserted"] > 0 and stats["points_combined"] > 0 and stats["keys_replayed"] == K
    snap = snapshot(st)
    assert_same(snap, r1_snapshot(engine, K, ALL, (k, t, v), op), "R1")
    assert_same(snap, r2_snapshot(K, ALL, (k, t, v), op), "R2")
    check_run_state(engine, st, (k, t, v), op)
    check_run_state(engine, st, (k, t, v), op, algos=("ARIMA",), emit=(False,))
    st.close()


# ---- 3. second resolution, sparse Stage 0 ----
def second_rows(K, n_batches, width, pts, seed):
    """second-resolution rows (two per point), a third of the keys alive only early, a third only late; 10 % of every batch's rows
    trail into the next batch"""
    rng = np.random.default_rng(seed)
    base = 1_000_000_000 + (orc.mix64(np.arange(K, dtype=np.uint64) + np.uint64(5)) % np.uint64(3_000_000_000)).astype(np.int64)
    raw = []
    for b in range(n_batches):
        g = np.arange(K) % 3
        alive = (g == 2) | ((g == 0) & (b < n_batches // 2)) | ((g == 1) & (b >= n_batches - 2))
        ks = np.nonzero(alive)[0].astype(np.uint64)
        pk = np.repeat(ks, pts)
        pt = np.concatenate([np.sort(rng.choice(width, pts, replace=False)) for _ in ks]).astype(np.int64) + T_BASE + b * width
        k, t = np.repeat(pk, 2), np.repeat(pt, 2)
        v = (np.repeat(base[pk.astype(np.int64)], 2) + rng.integers(-300_000_000, 300_000_000, size=k.size)).astype(np.uint64)
        order = rng.permutation(k.size)
        raw.append((k[order], t[order], v[order]))
    out, carry = [], None
    for b, (k, t, v) in enumerate(raw):
        late = rng.random(k.size) < 0.1 if b + 1 < n_batches else np.zeros(k.size, bool)
        parts = [(k[~late], t[~late], v[~late])] + ([carry] if carry is not None else [])
        out.append(cat(parts))
        carry = (k[late], t[late], v[late])
    return out


@pytest.mark.parametrize("plan,path", [({"sparse": "always", "sparse_sort": "lsd"}, 4), ({"sparse": "always", "sparse_sort": "partition", "stage0": "v2"}, 8)],
                         ids=["lsd", "partition"])
def test_second_resolution_sparse_stage0(engine, plan, path):
    K = 402
    batches = second_rows(K - 2, 4, 600, 5, seed=21)
    # key K - 2: its only points arrive late (in batch 2, at times of batch 0); key K - 1 first appears in a late row before every other point
    batches[2] = cat([batches[2], (np.array([K - 2, K - 2, K - 1], U64), np.array([T_BASE + 5, T_BASE + 9, T_BASE - 100], np.int64),
                                   np.array([7, 9, 11], U64))])
    batches[3] = cat([batches[3], (np.array([K - 1], U64), np.array([T_BASE + 2000], np.int64), np.array([5], U64))])
    st = new_state(engine, K)
    with engine.plan(**plan):
        for b, batch in enumerate(batches):
            stats = engine.merge_stream(st, *batch, value_op="sum")
            assert stats["stage0_path"] == path
            prev = cat(batches[:b]) if b else (np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64))
            assert_counts(stats, expected_counts(prev, batch, "sum"), b)
            if b:
                assert stats["points_inserted"] > 0 and stats["points_combined"] > 0 and stats["points_appended"] > 0
            sofar = cat(batches[:b + 1])
            snap = snapshot(st)
            assert_same(snap, r1_snapshot(engine, K, ALL, sofar, "sum"), (b, "R1"))
            assert_same(snap, r2_snapshot(K, ALL, sofar, "sum"), (b, "R2"))
    check_run_state(engine, st, cat(batches), "sum")
    st.close()


# ---- 4. long keys: several chunks of the merge kernel ----
def test_long_keys_late_points_in_every_chunk(engine):
    K, L = 503, 5000
    rng = np.random.default_rng(31)
    sk, st_, sv = orc.synth_rows(0, 6000, 500, 24)
    sk = sk + U64(3)
    lt = T_BASE + np.arange(L, dtype=np.int64) * 2          # even seconds: odd ones are free for inserts
    lk = np.repeat(np.arange(3, dtype=U64), L)
    ltt = np.tile(lt, 3)
    lv = rng.integers(1, 1 << 40, size=lk.size).astype(U64)
    first = cat([(sk, st_, sv), (lk, ltt, lv)])
    # late: inserts in the first, a middle and the last chunk, and a combine exactly at the first and at the last time
    pos = np.array([0, 10, 2047, 2048, 2500, 4095, 4096, 4990, L - 1])
    late_k = np.concatenate([np.repeat(np.arange(3, dtype=U64), pos.size), np.repeat(np.arange(3, dtype=U64), 2)])
    late_t = np.concatenate([np.tile(lt[pos] + 1, 3), np.tile(lt[[0, L - 1]], 3)])
    late_t[pos.size - 1] = lt[L - 1] - 1                     # key 0: not beyond the end (the others append one point)
    late_v = rng.integers(1, 1 << 40, size=late_k.size).astype(U64)
    late = (late_k, late_t, late_v)
    with engine.plan(sparse="always", sparse_sort="lsd"):
        for op in ("sum", "max"):
            st = new_state(engine, K)
            engine.merge_stream(st, *first, value_op=op)
            stats = engine.merge_stream(st, *late, value_op=op)
            assert_counts(stats, expected_counts(first, late, op), op)
            assert stats["points_combined"] == 6 and stats["points_appended"] == 2 and stats["keys_replayed"] == 3
            both = cat([first, late])
            snap = snapshot(st)
            assert_same(snap, r1_snapshot(engine, K, ALL, both, op), (op, "R1"))
            assert_same(snap, r2_snapshot(K, ALL, both, op), (op, "R2"))
            st.close()


# ---- 5. value edges ----
def test_value_edges(engine):
    K = 8
    t0 = T_BASE
    first = (np.arange(K, dtype=U64).repeat(3), np.tile(np.array([t0, t0 + 60, t0 + 120], np.int64), K),
             np.tile(np.array([(1 << 64) - 5, 1 << 50, (1 << 33) + 7], U64), K))
    late = (np.arange(K, dtype=U64).repeat(2), np.tile(np.array([t0, t0 + 60], np.int64), K), np.tile(np.array([9, (1 << 49) + 1], U64), K))
    for op in ("sum", "max"):
        st = new_state(engine, K)
        engine.merge_stream(st, *first, value_op=op)
        stats = engine.merge_stream(st, *late, value_op=op)
        assert stats["points_combined"] == 2 * K and stats["points_inserted"] == 0 and stats["keys_replayed"] == K
        vals = st.export_series()[1].reshape(K, 3)
        if op == "sum":
            assert (vals[:, 0] == U64(4)).all()                            # (2^64 - 5) + 9 wraps
            assert (vals[:, 1] == U64((1 << 50) + (1 << 49) + 1)).all()
        else:
            assert (vals[:, 0] == U64((1 << 64) - 5)).all() and (vals[:, 1] == U64(1 << 50)).all()   # the late value is smaller: unchanged
        both = cat([first, late])
        snap = snapshot(st)
        assert_same(snap, r1_snapshot(engine, K, ALL, both, op), (op, "R1"))
        assert_same(snap, r2_snapshot(K, ALL, both, op), (op, "R2"))
        st.close()


# ---- 6. in order: the append path ----
def test_in_order_batches_take_the_append_path(engine):
    K = 300
    k, t, v = orc.synth_rows(0, 60000, K, 48)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    a, twin = new_state(engine, K), new_state(engine, K)
    for lo, hi in ((0, 16), (16, 32), (32, 48)):
        sel = (bucket >= lo) & (bucket < hi)
        stats = engine.merge_stream(a, k[sel], t[sel], v[sel], value_op="sum")
        engine.run_stream(twin, k[sel], t[sel], v[sel], value_op="sum")
        assert stats["keys_replayed"] == stats["points_inserted"] == stats["points_combined"] == stats["points_too_old"] == 0
        assert stats["points_appended"] == stats["batch_points"] > 0 and stats["keys_touched"] > 0
        assert_same(snapshot(a), snapshot(twin), (lo, "twin"))
    a.close()
    twin.close()


# ---- 7. keep_from_t ----
def test_keep_from_drops_exactly_the_points_older_than_the_cut(engine):
    K = 300
    batches = lagged_batches()
    cut = int(orc.SYNTH_T_BASE + 30 * orc.SYNTH_T_STEP)   # the state holds buckets 0-31 by then; batch 4 carries rows of buckets 29-39
    for with_cut in (True, False):
        st = new_state(engine, K)
        for batch in batches[:4]:
            engine.merge_stream(st, *batch, value_op="sum")
        st.trim(keep_from=cut)
        seen = cat(batches[:4])
        kept = tuple(c[seen[1] >= cut] for c in seen)
        batch = batches[4]
        old_pts = orc.stage0(batch[0][batch[1] < cut], batch[1][batch[1] < cut], batch[2][batch[1] < cut], "sum")[0].size
        assert old_pts > 0
        stats = engine.merge_stream(st, *batch, value_op="sum", keep_from=cut if with_cut else 0)
        assert stats["points_too_old"] == (old_pts if with_cut else 0)
        assert_counts(stats, expected_counts(kept, batch, "sum", keep_from=cut if with_cut else 0), with_cut)
        new = tuple(c[batch[1] >= cut] for c in batch) if with_cut else batch
        assert_same(snapshot(st), r1_snapshot(engine, K, ALL, cat([kept, new]), "sum"), (with_cut, "R1"))
        if not with_cut:
            assert stats["points_inserted"] > 0                  # re-inserted before the window's first points
        st.close()


# ---- 8. interplay with stream batches, export / import, resize ----
def test_merge_then_stream_batches_export_import_and_resize(engine):
    K = 300
    batches = lagged_batches()
    k, t, v = cat(batches)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    head = tuple(c[bucket < 40] for c in (k, t, v))
    st = new_state(engine, K)
    for i in range(3):
        engine.merge_stream(st, head[0][i::3], head[1][i::3], head[2][i::3], value_op="sum")
    sofar = head
    for algo, lo, hi in (("DBSCAN", 40, 44), ("ARIMA", 44, 48)):
        sel = (bucket >= lo) & (bucket < hi)
        got = engine.run_stream(st, k[sel], t[sel], v[sel], value_op="sum", algo=algo)
        sofar = cat([sofar, (k[sel], t[sel], v[sel])])
        want = rows_of(engine.run(algo, *sofar, K, value_op="sum"))
        tmin = int(t[sel].min())
        m = want["flow_end_s"] >= tmin
        assert_rows(rows_of(got), {f: a[m] for f, a in want.items()}, algo)
        assert got["key_id"].size > 0
    with pytest.raises(TadError) as ei:       # tad_run_stream still refuses a late row
        engine.run_stream(st, head[0][:10], head[1][:10], head[2][:10], value_op="sum")
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT
    # export -> import into a fresh state -> merge again == no round trip
    snap = snapshot(st)
    st2 = new_state(engine, K)
    st2.load(snap["state"])
    st2.load_series(*snap["series"])
    st2.load_times(snap["times"])
    st2.load_history(*snap["history"])
    again = (head[0][::7], head[1][::7], head[2][::7])
    s1 = engine.merge_stream(st, *again, value_op="max")
    s2 = engine.merge_stream(st2, *again, value_op="max")
    assert s1["points_combined"] == s2["points_combined"] > 0
    assert_same(snapshot(st), snapshot(st2), "round trip")
    st2.close()
    # resize, then a merge that touches the new keys (late for the old ones)
    st.resize(K + 10)
    extra = (np.concatenate([np.arange(K, K + 10, dtype=U64), head[0][:50]]), np.concatenate([np.full(10, T_BASE + 77, np.int64), head[1][:50] + 1]),
             np.concatenate([np.arange(10, dtype=U64) + U64(100), head[2][:50]]))
    # (R1 over the window the state holds: it has seen sum and max batches by now)
    ln, vals = st.export_series()
    win = (np.repeat(np.arange(K + 10, dtype=U64), ln.astype(np.int64)), st.export_times(), vals)
    stats = engine.merge_stream(st, *extra, value_op="sum")
    assert stats["points_appended"] >= 10 and stats["points_inserted"] > 0
    assert_same(snapshot(st), r1_snapshot(engine, K + 10, ALL, cat([win, extra]), "sum"), "resize")
    st.close()


# ---- 9. refusals leave the state unchanged ----
def test_refusals_leave_the_state_unchanged(engine):
    K = 300
    batches = lagged_batches()
    st = new_state(engine, K)
    engine.merge_stream(st, *batches[0], value_op="sum")
    snap = snapshot(st)
    k, t, v = batches[1]
    bad = k.copy()
    bad[5] = K + 3
    with pytest.raises(TadError) as ei:
        engine.merge_stream(st, bad, t, v, value_op="sum")
    assert ei.value.code == _capi.TAD_ERR_KEY_RANGE
    assert_same(snapshot(st), snap, "key range")
    for kw in ({"num_keys": K + 1}, {"alpha": 1.5}):
        with pytest.raises(TadError) as ei:
            engine.merge_stream(st, k, t, v, value_op="sum", **kw)
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT, kw
        assert_same(snapshot(st), snap, kw)
    # TAD_FLAG_EMIT_ALL_POINTS through the C call itself
    kk, tt, vv = np.ascontiguousarray(k), np.ascontiguousarray(t), np.ascontiguousarray(v)
    job = _capi.Job(algo=0, value_op=_capi.TAD_OP["sum"], flags=_capi.TAD_FLAG_EMIT_ALL_POINTS)
    cols = _capi.Columns(n_rows=kk.size, key_id=kk.ctypes.data, flow_end_s=tt.ctypes.data, value=vv.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
    ms = _capi.MergeStats()
    assert engine._lib.tad_state_merge(engine._h, st._h, C.byref(job), C.byref(cols), 0, C.byref(ms)) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert engine._lib.tad_state_merge(engine._h, st._h, C.byref(job), C.byref(cols), 0, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert_same(snapshot(st), snap, "emit_all")
    # an empty batch: OK, stats zero, state untouched
    e = engine.merge_stream(st, np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64), value_op="sum")
    assert all(e[f] == 0 for f in ("rows_in", "batch_points", "points_appended", "points_inserted", "points_combined", "keys_touched", "keys_replayed"))
    assert_same(snapshot(st), snap, "empty")
    # states that cannot place a point by time
    for flags in (0, HIST, SER, HIST | SER):
        other = new_state(engine, K, flags)
        engine.run_stream(other, *batches[0], value_op="sum")
        osnap = snapshot(other)
        with pytest.raises(TadError) as ei:
            engine.merge_stream(other, k, t, v, value_op="sum")
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT, flags
        assert_same(snapshot(other), osnap, flags)
        other.close()
    # stale times: the series imported, the times not yet
    stale = new_state(engine, K)
    stale.load(snap["state"])
    stale.load_series(*snap["series"])
    with pytest.raises(TadError) as ei:
        engine.merge_stream(stale, k, t, v, value_op="sum")
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT
    stale.close()
    # and the state still merges afterwards; tad_run_stream still refuses the late rows
    engine.merge_stream(st, k, t, v, value_op="sum")
    assert_same(snapshot(st), r1_snapshot(engine, K, ALL, cat(batches[:2]), "sum"), "after refusals")
    with pytest.raises(TadError) as ei:
        engine.run_stream(st, *batches[0], value_op="sum")
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT
    st.close()


# ---- 10. narrow, device and two-key columns ----
def test_narrow_device_and_two_key_columns(engine):
    K = 300
    batches = lagged_batches()
    ref = new_state(engine, K)
    nar = new_state(engine, K)
    dev = new_state(engine, K)
    for k, t, v in batches:
        a = engine.merge_stream(ref, k, t, v, value_op="sum")
        b = engine.merge_stream(nar, k.astype(np.uint32), t.astype(np.uint32), v, value_op="sum")
        cols = [DeviceArray.from_host(engine, c) for c in (k, t, v)]
        c = engine.merge_stream(dev, *cols, value_op="sum")
        for f in ("points_inserted", "points_combined", "points_appended", "keys_replayed"):
            assert a[f] == b[f] == c[f], f
    assert_same(snapshot(nar), snapshot(ref), "narrow")
    assert_same(snapshot(dev), snapshot(ref), "device")
    assert_same(snapshot(ref), r1_snapshot(engine, K, ALL, cat(batches), "sum"), "R1")
    for s in (ref, nar, dev):
        s.close()
    # pod mode: the second keys carry the late points
    rng = np.random.default_rng(41)
    k, t, v = orc.synth_rows(0, 20000, K, 24)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    k2 = rng.integers(0, K, size=k.size).astype(U64)
    k2[rng.random(k.size) < 0.3] = U64(_capi.TAD_KEY_SKIP)
    first, second = bucket >= 8, bucket < 8
    st = new_state(engine, K)
    engine.merge_stream(st, k[first], t[first], v[first], agg_flow="pod", value_op="sum", key_id2=k2[first])
    only2 = np.full(int(second.sum()), _capi.TAD_KEY_SKIP, U64)
    stats = engine.merge_stream(st, only2, t[second], v[second], agg_flow="pod", value_op="sum", key_id2=k2[second])
    assert stats["points_inserted"] > 0 and stats["keys_replayed"] > 0
    both = (np.concatenate([k[first], only2]), np.concatenate([t[first], t[second]]), np.concatenate([v[first], v[second]]))
    both_k2 = np.concatenate([k2[first], k2[second]])
    assert_same(snapshot(st), r1_snapshot(engine, K, ALL, both, "sum", k2=both_k2), "pod")
    flat = (np.concatenate([both[0], both_k2]), np.concatenate([both[1], both[1]]), np.concatenate([both[2], both[2]]))
    assert_same(snapshot(st), r2_snapshot(K, ALL, flat, "sum"), "pod R2")
    st.close()


# ---- 11. concurrency ----
def test_merges_on_two_states_from_two_threads(engine):
    K = 300
    batches = lagged_batches()
    serial = []
    for op in ("sum", "max"):
        st = new_state(engine, K)
        for b in batches:
            engine.merge_stream(st, *b, value_op=op)
        serial.append(snapshot(st))
        st.close()
    states = [new_state(engine, K), new_state(engine, K)]
    errors, seen_rows = [], []

    def work(i, op):
        try:
            for b in batches:
                engine.merge_stream(states[i], *b, value_op=op)
        except Exception as exc:    # noqa: BLE001 (reported below)
            errors.append(exc)

    ths = [threading.Thread(target=work, args=(i, op)) for i, op in enumerate(("sum", "max"))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors
    for i in range(2):
        assert_same(snapshot(states[i]), serial[i], i)
    # run_state on A while B merges
    want = rows_of(engine.run_state(states[0], algo="EWMA"))
    b_state = new_state(engine, K)

    def merge_b():
        try:
            for b in batches:
                engine.merge_stream(b_state, *b, value_op="max")
        except Exception as exc:    # noqa: BLE001
            errors.append(exc)

    th = threading.Thread(target=merge_b)
    th.start()
    for _ in range(4):
        seen_rows.append(rows_of(engine.run_state(states[0], algo="EWMA")))
    th.join()
    assert not errors, errors
    for got in seen_rows:
        assert_rows(got, want, "run_state beside a merge")
    assert_same(snapshot(b_state), serial[1], "B")
    for s in states + [b_state]:
        s.close()


# ---- 12. Stage 0's retries inside a merge: an attempt that ends in a device error writes nothing that lasts ----
def test_wrong_lattice_hint_is_retried_and_leaves_the_same_state(engine):
    """the first attempt's Stage 0 raises the off-lattice error (seen inside the merge's own round trip, before anything is placed), the
    second derives the lattice: same state, same counters as a merge that needed one attempt"""
    K = 300
    batches = lagged_batches()
    a, twin = new_state(engine, K), new_state(engine, K)
    for b, batch in enumerate(batches[:3]):
        hint = (int(orc.SYNTH_T_BASE), 2 * int(orc.SYNTH_T_STEP), 24) if b else None     # every second bucket only: rows fall off it
        sa = engine.merge_stream(a, *batch, value_op="sum", lattice=hint)
        st = engine.merge_stream(twin, *batch, value_op="sum")
        assert sa["stage0_attempts"] == (2 if b else 1) and st["stage0_attempts"] == 1, (b, sa["stage0_attempts"], st["stage0_attempts"])
        for f in ("batch_points", "points_appended", "points_inserted", "points_combined", "keys_touched", "keys_replayed", "rows_used"):
            assert sa[f] == st[f], (b, f)
        if b:
            assert sa["points_inserted"] > 0 and sa["points_combined"] > 0
        assert_same(snapshot(a), snapshot(twin), (b, "twin"))
    sofar = cat(batches[:3])
    assert_same(snapshot(a), r1_snapshot(engine, K, ALL, sofar, "sum"), "R1")
    assert_same(snapshot(a), r2_snapshot(K, ALL, sofar, "sum"), "R2")
    check_run_state(engine, a, sofar, "sum")
    a.close()
    twin.close()


def halves_of_big_table(shift):
    """2.4e6 rows on 3000 keys x 100 buckets in two random halves (most points of the second half combine or insert); shift: added to
    every value"""
    K = 3000
    k, t, v = orc.synth_rows(0, 2_400_000, K, 100)
    v = v + U64(shift)
    order = np.random.default_rng(51).permutation(k.size)
    k, t, v = k[order], t[order], v[order]
    h = k.size // 2
    return K, [(k[:h], t[:h], v[:h]), (k[h:], t[h:], v[h:])]


@pytest.mark.parametrize("op", ["sum", "max"])
def test_partition_stage0_with_values_on_the_overflow_list(engine, op):
    """the dense partition Stage 0 (paths 2 / 3) in merge mode: a few values >= 2^49 take the overflow list, values >= 2^32 ride in the
    records; one attempt"""
    K, halves = halves_of_big_table(0)
    rng = np.random.default_rng(52)
    for i, (k, t, v) in enumerate(halves):
        v = v.copy()
        big = rng.random(v.size) < 0.003
        v[big] = rng.integers(2**50, 2**62, size=int(big.sum()), dtype=np.uint64)
        wide = rng.random(v.size) < 0.02
        v[wide] = v[wide] + U64(2**32)
        halves[i] = (k, t, v)
    st = new_state(engine, K)
    with engine.plan(stage0="v2"):
        for b, batch in enumerate(halves):
            stats = engine.merge_stream(st, *batch, value_op=op)
            assert stats["stage0_path"] in (2, 3) and stats["stage0_attempts"] == 1, (b, stats["stage0_path"], stats["stage0_attempts"])
            prev = halves[0] if b else (np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64))
            assert_counts(stats, expected_counts(prev, batch, op), b)
        assert stats["points_combined"] > 0 and stats["keys_replayed"] == K
    both = cat(halves)
    snap = snapshot(st)
    assert_same(snap, r1_snapshot(engine, K, ALL, both, op), "R1")
    assert_same(snap, r2_snapshot(K, ALL, both, op), "R2")
    st.close()


def test_overflow_list_full_is_retried_on_the_scatter_path(engine):
    """more than 2^20 values >= 2^49 in a batch: the partition Stage 0 gives up (the merge sees the error word and places nothing), the
    direct scatter redoes the batch — attempts 2, path 1 — and the state is the one a merge that went the scatter path at once leaves"""
    K, halves = halves_of_big_table(2**50)
    a, twin = new_state(engine, K), new_state(engine, K)
    for b, batch in enumerate(halves):
        with engine.plan(stage0="v2"):
            sa = engine.merge_stream(a, *batch, value_op="sum")
        with engine.plan(stage0="v1"):
            st = engine.merge_stream(twin, *batch, value_op="sum")
        assert (sa["stage0_attempts"], sa["stage0_path"]) == (2, 1), (b, sa["stage0_attempts"], sa["stage0_path"])
        assert (st["stage0_attempts"], st["stage0_path"]) == (1, 1), (b, st["stage0_attempts"], st["stage0_path"])
        prev = halves[0] if b else (np.zeros(0, U64), np.zeros(0, np.int64), np.zeros(0, U64))
        want = expected_counts(prev, batch, "sum")
        assert_counts(sa, want, (b, "retried"))
        assert_counts(st, want, (b, "twin"))
        assert_same(snapshot(a), snapshot(twin), (b, "twin"))
    assert sa["points_combined"] > 0 and sa["keys_replayed"] == K
    both = cat(halves)
    assert_same(snapshot(a), r1_snapshot(engine, K, ALL, both, "sum"), "R1")
    assert_same(snapshot(a), r2_snapshot(K, ALL, both, "sum"), "R2")
    a.close()
    twin.close()


# ---- 13. stats == NULL on a merge that does its work ----
def test_a_successful_merge_without_stats(engine):
    K = 300
    batches = lagged_batches()
    a, twin = new_state(engine, K), new_state(engine, K)
    for batch in batches[:2]:
        k, t, v = (np.ascontiguousarray(c) for c in batch)
        job = _capi.Job(algo=0, value_op=_capi.TAD_OP["sum"])
        cols = _capi.Columns(n_rows=k.size, key_id=k.ctypes.data, flow_end_s=t.ctypes.data, value=v.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
        assert engine._lib.tad_state_merge(engine._h, a._h, C.byref(job), C.byref(cols), 0, None) == _capi.TAD_OK
        engine.merge_stream(twin, k, t, v, value_op="sum")
    assert_same(snapshot(a), snapshot(twin), "no stats")
    assert_same(snapshot(a), r1_snapshot(engine, K, ALL, cat(batches[:2]), "sum"), "R1")
    a.close()
    twin.close()
