"""GPU: retiring dead keys (tad_state_compact / tad_keydict_compact, include/tad.h).  The defining property: a compaction moves what the
survivors hold and recomputes nothing, so every expected value here is a numpy selection over the exports taken BEFORE the call, compared
as bits — remap, every field of tad_compact_stats, moments, history, series and times; later batches, merges, trims and tad_run_state on
the compacted state equal those on an uncompacted twin with the key ids passed through remap; the dictionary afterwards is the one a fresh
dictionary holds after importing the surviving tuples.  A refused call leaves state and dictionary as they were."""
import os
import re

import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import ROOT, host
from state_helpers import HIST, SER, STATE_FIELDS, TIMES, U64, assert_rows, assert_same, bits, new_state, rows_of, snapshot

pytestmark = pytest.mark.gpu

SKIP = np.uint64(capi.TAD_KEY_SKIP)
CUT = 1_700_000_000          # the time rule of every case: a key whose newest point is older is idle


def scan_tile():
    """launch_scan's tile (tad_kernels.hip): the key counts around it are boundaries of the new ids' scan"""
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_kernels.hip")).read()
    block = int(re.search(r"static constexpr int kBlock = (\d+);", src).group(1))
    items = int(re.search(r"static constexpr int kScanItems = (\d+);", src).group(1))
    assert re.search(r"kScanTile = kBlock \* kScanItems;", src)
    return block * items


def build_state(engine, flags, n, last_t, seed):
    """a state with n[k] points per key ending at last_t[k], through the imports: arbitrary moments, random values, times one second
    apart, the history = the series' values sorted"""
    rng = np.random.default_rng(seed)
    K = n.size
    n = n.astype(np.int64)
    st = new_state(engine, K, flags)
    seen = n > 0
    st.load({"n": n.astype(np.uint32), "avg": np.where(seen, rng.random(K) * 1e9, 0.0), "m2": np.where(seen, rng.random(K) * 1e15, 0.0),
             "ewma": np.where(seen, rng.random(K) * 1e9, 0.0), "last_t": np.where(seen, last_t, 0).astype(np.int64)})
    total = int(n.sum())
    vals = rng.integers(1, 1 << 40, size=total).astype(U64)
    key = np.repeat(np.arange(K), n)
    end = np.repeat(np.cumsum(n), n)
    if flags & SER:
        st.load_series(n.astype(U64), vals)
    if flags & TIMES:
        st.load_times((np.repeat(last_t, n) - (end - 1 - np.arange(total))).astype(np.int64))
    if flags & HIST:
        st.load_history(n.astype(U64), vals[np.lexsort((vals, key))])
    return st


def select(snap, live):
    """the exports of a fresh state that imported the survivors' exports: max(m, 1) keys, the one key of m == 0 unseen"""
    m = int(live.sum())
    out = {"state": {f: (snap["state"][f][live] if m else np.zeros(1, snap["state"][f].dtype)) for f in STATE_FIELDS}, "history": None, "series": None,
           "times": None}
    for part in ("history", "series"):
        if snap[part] is not None:
            ln, vals = snap[part]
            out[part] = (ln[live] if m else np.zeros(1, U64), vals[np.repeat(live, ln.astype(np.int64))])
    if snap["times"] is not None:
        times = snap["times"][np.repeat(live, snap["series"][0].astype(np.int64))]
        out["times"] = times if times.size else None      # (a state without points exports no times)
    return out


def expected_remap(live):
    return np.where(live, np.cumsum(live) - 1, -1).astype(np.int64).astype(U64)      # -1 -> TAD_KEY_SKIP


def liveness(pattern, K, rng):
    if pattern == "all_live":
        return np.ones(K, bool)
    if pattern == "all_retired":
        return np.zeros(K, bool)
    if pattern == "alternating":
        return np.arange(K) % 2 == 0
    live = rng.random(K) < 0.5
    if pattern == "ends_retired":
        live[0] = live[-1] = False
    elif pattern == "ends_live":
        live[0] = live[-1] = True
    else:
        assert pattern == "runs" and K >= 400
        live[5:5 + 133] = False
        live[201:201 + 131] = True
    return live


def longest_run(mask):
    """(start, length) of the longest run of True"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    starts, ends = edges[::2], edges[1::2]
    i = int(np.argmax(ends - starts))
    return int(starts[i]), int(ends[i] - starts[i])


def check_pattern(pattern, live):
    K = live.size
    if pattern == "all_live":
        assert live.all()
    elif pattern == "all_retired":
        assert not live.any()
    elif pattern == "alternating":
        assert K < 2 or (live[::2].all() and not live[1::2].any())
    elif pattern == "ends_retired":
        assert not live[0] and not live[-1] and live.any()
    elif pattern == "ends_live":
        assert live[0] and live[-1] and not live.all()
    else:
        for mask in (~live, live):
            start, length = longest_run(mask)
            assert length >= 130 and start % 64 != 0 and (start + length) % 64 != 0, (start, length)


TILE = scan_tile()
CASES = [   # (K, flags, rule, pattern): every K, every flag set, every rule and every pattern at least once
    (1, 0, "unseen", "all_retired"), (1, 11, "idle", "all_live"), (1, 3, "idle", "all_retired"),
    (63, 1, "idle", "alternating"), (64, 2, "unseen", "ends_retired"), (65, 3, "both", "ends_live"), (65, 0, "both", "all_live"),
    (2047, 10, "both", "runs"), (2048, 11, "idle", "runs"), (2048, 11, "idle", "all_retired"), (2049, 0, "both", "alternating"),
    (2049, 11, "trim", "ends_retired"), (2049, 11, "unseen", "all_live"),
    (4097, 11, "both", "runs"), (4097, 1, "unseen", "ends_live"), (4097, 10, "trim", "alternating"), (4097, 3, "unseen", "all_retired"),
    (70_001, 11, "both", "runs"), (70_001, 0, "idle", "ends_retired"), (70_001, 3, "unseen", "alternating"), (70_001, 2, "idle", "runs"),
] + ([(TILE + d, 11, "both", "runs") for d in (-1, 0, 1)] if TILE != 2048 else [])


def test_the_cases_cover_every_flag_rule_and_key_count():
    assert {c[1] for c in CASES} == {0, 1, 2, 3, 10, 11}
    assert {c[2] for c in CASES} >= {"unseen", "idle", "both", "trim"}
    assert {c[0] for c in CASES} >= {1, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001, TILE - 1, TILE, TILE + 1}
    assert {c[3] for c in CASES} == {"alternating", "ends_retired", "ends_live", "runs", "all_live", "all_retired"}


# ---- 1. the exports afterwards are the selection of the exports before ----
@pytest.mark.parametrize("K,flags,rule,pattern", CASES)
def test_exports_after_a_compaction_are_the_survivors_exports(engine, K, flags, rule, pattern):
    rng = np.random.default_rng(K * 131 + flags * 7 + len(rule) + len(pattern))
    want_live = liveness(pattern, K, rng)
    n = rng.integers(1, 6, size=K)
    last_t = np.where(want_live, CUT + 10 + rng.integers(0, 100, size=K), CUT - 1 - rng.integers(0, 100, size=K))
    dead = np.flatnonzero(~want_live)
    if rule == "unseen":
        n[dead] = 0                                   # never fed
    elif rule in ("both", "trim"):
        n[dead[::2]] = 0                              # every other dead key never fed; the rest idle (both) or emptied by the trim below (trim)
    st = build_state(engine, flags, n, last_t, K + flags)
    if rule == "trim":
        assert flags & SER and flags & TIMES
        fed_dead = int((n[dead] > 0).sum())
        assert st.trim(keep_from=CUT) == int(n[dead].sum()) and (fed_dead > 0 or dead.size < 2)
    rb = CUT if rule in ("idle", "both") else 0
    snap = snapshot(st)
    sn, slt = snap["state"]["n"], snap["state"]["last_t"]
    live = (sn > 0) & ((rb == 0) | (slt >= rb))
    assert np.array_equal(live, want_live)
    check_pattern(pattern, live)
    m = int(live.sum())
    unseen, idle = sn == 0, (sn > 0) & ~live
    if rule == "both" and dead.size >= 2:
        assert unseen.any() and idle.any()
    if rule == "trim":
        assert not idle.any() and int(unseen.sum()) == dead.size
    dropped = int(sn[idle].sum())
    bytes_before = st.nbytes()
    remap, stats = st.compact(rb, out="device" if K == 4097 else "host")
    if K == 4097:
        remap = remap.to_host()
    assert np.array_equal(remap, expected_remap(live))
    kept_points = int(sn[live].sum())
    want = {"keys_before": K, "keys_after": m, "num_keys": max(m, 1), "keys_unseen": int(unseen.sum()), "keys_idle": int(idle.sum()), "points_dropped": dropped,
            "series_points_moved": kept_points if (flags & SER and dropped) else 0, "history_points_moved": kept_points if (flags & HIST and dropped) else 0,
            "bytes_before": bytes_before, "bytes_after": st.nbytes()}
    assert {f: stats[f] for f in want} == want
    assert stats["job_context"] >= 0 and stats["ms_total"] >= 0.0
    assert st.num_keys == max(m, 1)
    assert_same(snapshot(st), select(snap, live), (K, flags, rule, pattern))
    if pattern == "all_live":
        assert np.array_equal(remap, np.arange(K, dtype=U64)) and stats["bytes_after"] == bytes_before
    if pattern == "all_retired":
        assert st.num_keys == 1 and (remap == SKIP).all() and st.export()["n"][0] == 0
    if not dropped and m < K and K > 1:              # only unseen keys went: the arenas stay, the moment blocks and offsets shrink
        assert stats["bytes_after"] < bytes_before
    # a second compaction finds nothing to retire (the m == 0 state keeps its one unseen key: it goes and comes back)
    remap2, stats2 = st.compact(rb)
    if m:
        assert np.array_equal(remap2, np.arange(m, dtype=U64)) and stats2["keys_after"] == stats2["keys_before"] == m and stats2["bytes_after"] == stats["bytes_after"]
    assert_same(snapshot(st), select(snap, live), "again")
    st.close()


# ---- 2. segments around kHistChunk between retired neighbours ----
@pytest.mark.parametrize("flags", [11, 1])
def test_segments_around_the_chunk_size_move_whole(engine, flags):
    lens = [2049, 2047, 2049, 0, 2048, 2049, 2049, 0, 2049, 4100, 2049]
    old = np.array([1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1], bool)             # the 2049-point neighbours of the survivors are idle
    n = np.array(lens)
    assert [lens[i] for i in np.flatnonzero(~old & (n > 0))] == [2047, 2048, 2049, 4100] and (n[old] == 2049).all()
    last_t = np.where(old, CUT - 5, CUT + 5000)
    st = build_state(engine, flags, n, last_t, 99 + flags)
    snap = snapshot(st)
    remap, stats = st.compact(0)                                         # only the two unseen keys go: nothing moves
    live0 = n > 0
    assert np.array_equal(remap, expected_remap(live0)) and stats["keys_unseen"] == 2 and stats["keys_idle"] == 0 and stats["points_dropped"] == 0
    assert stats["series_points_moved"] == 0 and stats["history_points_moved"] == 0
    snap0 = select(snap, live0)
    assert_same(snapshot(st), snap0, "unseen only")
    live1 = ~old[live0]
    remap, stats = st.compact(CUT)
    survivors = 2047 + 2048 + 2049 + 4100
    assert np.array_equal(remap, expected_remap(live1)) and stats["keys_idle"] == 5 and stats["points_dropped"] == 5 * 2049
    assert stats["series_points_moved"] == (survivors if flags & SER else 0) and stats["history_points_moved"] == survivors
    assert_same(snapshot(st), select(snap0, live1), "idle")
    st.close()


# ---- 3. life goes on: the compacted state and an uncompacted twin take the same further batches ----


def mapped(rows, remap_ext):
    """the twin's rows without the retired keys' rows, key ids through remap"""
    new = remap_ext[rows["key_id"].astype(np.int64)]
    keep = new != SKIP
    out = {f: a[keep] for f, a in rows.items()}
    out["key_id"] = new[keep].astype(rows["key_id"].dtype)
    return out, int((~keep).sum())


@pytest.mark.parametrize("flags", [11, 3])
def test_later_calls_equal_the_uncompacted_twin_through_remap(engine, flags):
    rng = np.random.default_rng(5 + flags)
    K0, T0 = 300, CUT - 50
    old = np.arange(K0) % 3 == 1                                          # these keys stop early: idle at the compaction
    keys = np.arange(K0, dtype=U64)

    def batch(ks, t_lo, pts, step=2):
        k = np.repeat(ks, pts)
        t = np.tile(t_lo + step * np.arange(pts), ks.size).astype(np.int64)
        return k, t, rng.integers(1000, 1 << 30, size=k.size).astype(U64)

    first = [np.concatenate(x) for x in zip(batch(keys[old], T0, 8), batch(keys[~old], CUT + 10, 8))]      # even seconds only
    a, b = new_state(engine, K0, flags), new_state(engine, K0, flags)      # a is compacted, b is the twin
    for st in (a, b):
        engine.run_stream(st, *first, value_op="max")
    snap = snapshot(a)
    remap, stats = a.compact(CUT)
    m = int((~old).sum())
    assert np.array_equal(remap, expected_remap(~old)) and stats["keys_idle"] == K0 - m and stats["points_dropped"] == 8 * (K0 - m)
    assert_same(snapshot(a), select(snap, ~old), "compacted")
    retired_rows = 0
    n_new = 0
    for i, algo in enumerate(("EWMA", "DBSCAN", "ARIMA")):
        # rows for most old keys (the retired ones among them), and 20 new keys appended on both states
        ks = np.concatenate([keys[rng.random(K0) < 0.8], K0 + n_new + np.arange(20, dtype=U64)])
        n_new += 20
        kb, tb, vb = batch(ks, CUT + 100 * (i + 1), 3)
        remap_ext = np.concatenate([remap, m + np.arange(n_new, dtype=U64)])
        b.resize(K0 + n_new)
        a.resize(m + n_new)
        kw = dict(value_op="max", algo=algo, emit_all=True, eps=5e8, min_samples=3)
        want, cut_rows = mapped(rows_of(engine.run_stream(b, kb, tb, vb, **kw)), remap_ext)
        got = rows_of(engine.run_stream(a, remap_ext[kb.astype(np.int64)], tb, vb, **kw))
        retired_rows += cut_rows
        assert got["key_id"].size > 0
        assert_rows(got, want, algo)
    assert retired_rows > 0                                               # a retired key had rows in the twin
    if flags & TIMES:
        late = batch(keys[rng.random(K0) < 0.5], CUT + 11, 4)             # odd seconds inside the first batch's range: inserted
        sa = engine.merge_stream(a, remap_ext[late[0].astype(np.int64)], late[1], late[2], value_op="max")
        sb = engine.merge_stream(b, *late, value_op="max")
        assert sa["points_inserted"] > 0 and sb["points_inserted"] > sa["points_inserted"]
        for st in (a, b):
            assert st.trim(keep_from=CUT + 14) > 0
        for algo in ("EWMA", "DBSCAN", "ARIMA"):
            for emit_all in (False, True):
                kw = dict(algo=algo, emit_all=emit_all, eps=5e8, min_samples=3)
                want, cut_rows = mapped(rows_of(engine.run_state(b, **kw)), remap_ext)
                assert cut_rows > 0 or not (emit_all and algo == "EWMA")
                assert_rows(rows_of(engine.run_state(a, **kw)), want, ("run_state", algo, emit_all))
    assert_same(snapshot(a), select(snapshot(b), remap_ext != SKIP), "the end")
    a.close(), b.close()


# ---- 4. the dictionary ----


def tuples(rng, n, salt):
    """n distinct two-column tuples with negative and large values"""
    i = np.arange(n, dtype=np.int64) + salt
    return [i * -977, (i % 11) + (np.int64(1) << 40)]


@pytest.mark.parametrize("sides", [1, 2])
def test_dictionary_compaction_equals_an_import_of_the_survivors(engine, sides):
    rng = np.random.default_rng(40 + sides)
    n = 5000 // sides
    ta, tb = tuples(rng, n, 0), (tuples(rng, n, 7) if sides == 2 else None)            # (side b shares most of side a's values: the side is part of the tuple)
    d = engine.key_dict(2, 1)
    k1, k2, _, before = d.encode(ta, None, tb, None)
    K = d.num_keys()
    assert before == 0 and K == n * sides
    cols0, side0 = d.export()
    live = np.zeros(K, bool)
    live[rng.choice(K, size=100, replace=False)] = True
    remap = expected_remap(live)
    bytes0 = d.nbytes()
    assert d.compact(remap) == 100 == d.num_keys()
    assert d.nbytes() < bytes0
    cols1, side1 = d.export()
    assert all(np.array_equal(c1, c0[live]) for c1, c0 in zip(cols1, cols0)) and np.array_equal(side1, side0[live])
    fresh = engine.key_dict(2, 200)                                                     # what tad_keydict_create(expected_keys = 2 m) holds after the import
    fresh.load([c[live] for c in cols0], side0[live])
    assert d.nbytes() == fresh.nbytes()
    l1, l2 = d.lookup(ta, None, tb, None)
    f1, f2 = fresh.lookup(ta, None, tb, None)
    assert np.array_equal(l1, remap[k1.astype(np.int64)]) and np.array_equal(l1, f1)    # a retired tuple looks up to TAD_KEY_SKIP
    if sides == 2:
        assert np.array_equal(l2, remap[k2.astype(np.int64)]) and np.array_equal(l2, f2)
    assert (l1 == SKIP).any() and (l1 != SKIP).any()
    # one batch of survivors, retired tuples and new tuples: survivors keep remap's ids, the others get m, m + 1, ... as they appear
    fresh_t = tuples(rng, 300, 1_000_000)
    pick = rng.permutation(n)[:600]
    mix = [np.concatenate([ta[c][pick[:300]], fresh_t[c], ta[c][pick[300:]]]) for c in range(2)]
    old_ids = np.concatenate([remap[k1.astype(np.int64)][pick[:300]], np.full(300, SKIP), remap[k1.astype(np.int64)][pick[300:]]])
    want, nxt, seen = np.empty(900, U64), 100, {}
    for i in range(900):
        if old_ids[i] != SKIP:
            want[i] = old_ids[i]
        else:
            t = (int(mix[0][i]), int(mix[1][i]))
            if t not in seen:
                seen[t] = nxt
                nxt += 1
            want[i] = seen[t]
    assert (old_ids == SKIP).sum() > 300 and (old_ids != SKIP).any()
    for dd in (d, fresh):
        ids, _, fr, before = dd.encode(mix)
        assert before == 100 and np.array_equal(ids, want) and dd.num_keys() == nxt
    # growth after the compaction keeps every id
    more = tuples(rng, 3000, 2_000_000)
    ids, _, _, before = d.encode(more)
    assert before == nxt and np.array_equal(ids, nxt + np.arange(3000, dtype=U64))
    assert np.array_equal(d.lookup(mix)[0], want)
    l1, _ = d.lookup(ta, None, tb, None)
    kept = remap[k1.astype(np.int64)] != SKIP
    assert np.array_equal(l1[kept], remap[k1.astype(np.int64)][kept])
    # ... and to nothing: an empty dictionary at the smallest size, which starts over at id 0
    bytes1 = d.nbytes()
    assert d.compact(np.full(d.num_keys(), SKIP, U64)) == 0 == d.num_keys()
    smallest = engine.key_dict(2, 1)
    assert d.nbytes() == smallest.nbytes() <= bytes1
    assert (host(d.lookup(ta)[0]) == SKIP).all() and d.export()[1].size == 0
    ids, _, _, before = d.encode([c[:50] for c in ta])
    assert before == 0 and np.array_equal(ids, np.arange(50, dtype=U64))
    b2 = d.nbytes()
    assert d.compact(np.arange(50, dtype=U64)) == 50 and d.nbytes() <= b2                # the identity: nothing leaves, nothing grows
    d.close(), fresh.close(), smallest.close()


def test_dictionary_takes_a_remap_in_device_memory(engine):
    d = engine.key_dict(1, 1)
    col = [np.arange(1000, dtype=np.int64) * 3]
    d.encode(col)
    live = np.arange(1000) % 7 != 0
    remap = expected_remap(live)
    assert d.compact(DeviceArray.from_host(engine, remap)) == int(live.sum())
    assert np.array_equal(d.lookup(col)[0], remap) and np.array_equal(d.export()[0][0], col[0][live])
    d.close()


# ---- 5. refusals leave everything unchanged ----
def kd_snapshot(d):
    cols, side = d.export()
    return d.num_keys(), [c.copy() for c in cols], side.copy(), d.nbytes()


def assert_kd_unchanged(d, snap, col, ids, what):
    n, cols, side, nbytes = kd_snapshot(d)
    assert n == snap[0] and nbytes == snap[3], what
    assert all(np.array_equal(a, b) for a, b in zip(cols, snap[1])) and np.array_equal(side, snap[2]), what
    assert np.array_equal(d.lookup(col)[0], ids), what


def test_a_remap_that_is_not_a_compaction_is_refused(engine):
    d = engine.key_dict(1, 1)
    col = [np.arange(1000, dtype=np.int64) * -5]
    ids = d.encode(col)[0]
    snap = kd_snapshot(d)
    live = np.arange(1000) % 3 != 0
    good = expected_remap(live)
    m = int(live.sum())
    kept = np.flatnonzero(live)
    swapped, dup, gap, high = good.copy(), good.copy(), good.copy(), good.copy()
    swapped[kept[10]], swapped[kept[11]] = good[kept[11]], good[kept[10]]
    dup[kept[500]] = good[kept[499]]
    gap[kept[300]:] = np.where(gap[kept[300]:] != SKIP, gap[kept[300]:] + U64(1), SKIP)      # ..., 299, 301, ...: the last entry is m
    high[kept[-1]] = U64(m)
    assert gap[gap != SKIP].max() == m
    for what, r in (("short", good[:-1]), ("long", np.append(good, SKIP)), ("swapped", swapped), ("duplicate", dup), ("gap", gap), ("value >= m", high),
                    ("descending", good[::-1].copy())):
        with pytest.raises(TadError) as ei:
            d.compact(r)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT, what
        assert_kd_unchanged(d, snap, col, ids, what)
    assert engine._lib.tad_keydict_compact(engine._h, d._h, None, 1000, capi.TAD_MEM_HOST, None) == capi.TAD_ERR_INVALID_ARGUMENT
    assert engine._lib.tad_keydict_compact(engine._h, d._h, good.ctypes.data, 1000, 7, None) == capi.TAD_ERR_INVALID_ARGUMENT      # no such memory
    assert_kd_unchanged(d, snap, col, ids, "NULL")
    assert d.compact(good) == m                                                                # the same remap, passed properly
    d.close()


def test_a_state_refuses_a_null_remap_and_stale_times(engine):
    n = np.array([3, 0, 2, 4, 0, 1])
    last_t = np.full(6, CUT + 50)
    st = build_state(engine, 11, n, last_t, 3)
    snap = snapshot(st)
    assert engine._lib.tad_state_compact(engine._h, st._h, 0, None, capi.TAD_MEM_HOST, None) == capi.TAD_ERR_INVALID_ARGUMENT
    buf = np.full(6, 7, U64)
    assert engine._lib.tad_state_compact(engine._h, st._h, 0, buf.ctypes.data, 7, None) == capi.TAD_ERR_INVALID_ARGUMENT and (buf == 7).all()
    assert_same(snapshot(st), snap, "NULL remap")
    st.load_series(*snap["series"])                                       # the times that go with the series have not come yet
    with pytest.raises(TadError) as ei:
        st.compact(0)
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "times" in ei.value.message and st.num_keys == 6
    with pytest.raises(TadError):
        st.trim(keep_points=1)                                            # as a trim refuses it
    st.load_times(snap["times"])
    assert_same(snapshot(st), snap, "stale times")
    remap, stats = st.compact(0)
    assert np.array_equal(remap, expected_remap(n > 0)) and stats["keys_after"] == 4
    assert_same(snapshot(st), select(snap, n > 0), "afterwards")
    st.close()


def test_workspace_limit_refuses_a_big_compaction_and_leaves_everything_unchanged(engine):
    """Scratch (include/tad.h): about 68 B per key of the state plus 8 B per key of a host remap; the dictionary's call needs 12 B per key
    plus 8 for a host remap.  With a limit of 1 MiB, 100 000 keys need 7.6 MB and 2 MB: both refused before anything is touched; 1000 keys
    need under 100 KB and pass."""
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    try:
        K = 100_000
        n = (np.arange(K) % 2).astype(np.int64)
        st = build_state(small, 0, n, np.full(K, CUT + 5), 8)
        snap, nbytes = snapshot(st), st.nbytes()
        with pytest.raises(TadError) as ei:
            st.compact(0)
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE and st.num_keys == K and st.nbytes() == nbytes
        assert_same(snapshot(st), snap, "state")
        d = small.key_dict(1, 1)
        col = [np.arange(K, dtype=np.int64)]
        d.load(col)
        ksnap = kd_snapshot(d)
        with pytest.raises(TadError) as ei:
            d.compact(expected_remap(n > 0))
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        assert_kd_unchanged(d, ksnap, [col[0][:5000]], np.arange(5000, dtype=U64), "dictionary")
        st.close(), d.close()
        n = (np.arange(1000) % 2).astype(np.int64)
        st = build_state(small, 3, n, np.full(1000, CUT + 5), 9)
        d = small.key_dict(1, 1)
        d.load([np.arange(1000, dtype=np.int64)])
        remap, stats = st.compact(0)
        assert stats["keys_after"] == 500 and d.compact(remap) == 500
        st.close(), d.close()
    finally:
        small.close()


# ---- 6. end to end: stream through the dictionary, trim and compact on a tick, ask the state for the window's verdicts ----
def test_streaming_ingest_with_compactions_equals_the_batch_job_over_the_window(engine):
    """test_gpu_keydict's end-to-end table, with keys that live only for a stretch of the time span (a sliding range of connections, and
    twenty keys that come back at the end), in arrival order with a few late rows, cut into eight batches.  Per batch: encode ->
    tad_state_resize -> tad_state_merge(keep_from); after batches 3 and 6: trim to the newest `window` seconds, compact the state, compact
    the dictionary.  tad_run_state then returns exactly the rows of tad_run over the raw rows inside the final window — compared by key
    TUPLE: once keys have been retired the ids differ from those of one factorisation."""
    rng = np.random.default_rng(78)
    n, nkeys, span, window = 48_000, 3000, 7200, 1200
    pos = np.arange(n)
    hi = 40 + (nkeys - 40) * pos // n                                            # the connections a row can belong to slide with time
    lo = np.maximum(hi - 500, 20)
    kidx = (lo + rng.random(n) * (hi - lo)).astype(np.int64)
    back = (rng.random(n) < 0.02) & ((pos < n // 10) | (pos > n * 9 // 10))      # keys 0..19: at the start, and again at the end
    kidx = np.where(back, rng.integers(0, 20, size=n), kidx)
    t = orc.SYNTH_T_BASE + pos * span // n + rng.integers(0, 3, size=n)
    late = rng.random(n) < 0.01
    t = np.where(late, np.maximum(t - rng.integers(60, 600, size=n), orc.SYNTH_T_BASE), t).astype(np.int64)
    v = rng.integers(1, 1 << 30, size=n).astype(U64)
    v[rng.random(n) < 0.002] += U64(1 << 36)
    cols = [kidx % 13, (kidx % 7) * -977, kidx // 91, kidx % 3 + (1 << 40), kidx % 2, kidx * 31 % 5]       # (kidx -> tuple is injective)
    cols = [c.astype(np.int64) for c in cols]
    d = engine.key_dict(6, 1)
    st = engine.state_create(1, history=True, series=True, times=True)
    edges = [0, 4000, 10_000, 16_000, 22_000, 28_000, 34_000, 41_000, n]
    keep_from, retired_kidx, returned = 0, set(), set()
    kidx_of_id = np.zeros(0, np.int64)                                           # the host's key table: id -> connection
    for b, (e0, e1) in enumerate(zip(edges[:-1], edges[1:])):
        ids, _, fr, before = d.encode([c[e0:e1] for c in cols])
        kidx_of_id = np.concatenate([kidx_of_id[:before], kidx[e0:e1][fr.astype(np.int64)]])
        returned |= retired_kidx & set(kidx[e0:e1][fr.astype(np.int64)].tolist())
        if d.num_keys() > st.num_keys:
            st.resize(d.num_keys())
        engine.merge_stream(st, ids, t[e0:e1], v[e0:e1], value_op="sum", keep_from=keep_from)
        if b in (2, 5):                                                          # the tick after batches 3 and 6
            keep_from = int(t[:e1].max()) - window
            st.trim(keep_from=keep_from)
            sn = st.export()["n"]
            dead = sn == 0
            remap, stats = st.compact(0)
            assert 0 < int(dead.sum()) == stats["keys_unseen"] < sn.size and stats["keys_after"] > 0
            assert np.array_equal(remap, expected_remap(~dead))
            assert d.compact(remap) == stats["keys_after"] == st.num_keys
            retired_kidx |= set(kidx_of_id[dead].tolist())
            kidx_of_id = kidx_of_id[~dead]                                       # remap applied to the host's key table
    assert returned                                                              # a tuple was retired and came back under a new id
    assert d.num_keys() == st.num_keys == kidx_of_id.size
    dcols, _ = d.export()
    assert all(np.array_equal(dc, c) for dc, c in zip(dcols, [kidx_of_id % 13, (kidx_of_id % 7) * -977, kidx_of_id // 91, kidx_of_id % 3 + (1 << 40),
                                                                kidx_of_id % 2, kidx_of_id * 31 % 5]))
    sel = t >= keep_from
    ref_ids, _, ref_first = engine.factorize([c[sel] for c in cols])
    ref_kidx = kidx[sel][ref_first.astype(np.int64)]

    def by_tuple(res, kidx_table):
        r = rows_of(res)
        conn = kidx_table[r.pop("key_id").astype(np.int64)]
        order = np.lexsort((r["flow_end_s"], conn))
        r["connection"] = conn
        return {f: a[order] for f, a in r.items()}

    for algo in ("EWMA", "DBSCAN"):
        for emit_all in (False, True):
            got = by_tuple(engine.run_state(st, algo=algo, emit_all=emit_all), kidx_of_id)
            want = by_tuple(engine.run(algo, ref_ids, t[sel], v[sel], ref_first.size, value_op="sum", emit_all=emit_all), ref_kidx)
            assert got["connection"].size == want["connection"].size > 0, (algo, emit_all)
            for f in want:
                assert np.array_equal(bits(got[f]), bits(want[f])), (algo, emit_all, f)
    st.close(), d.close()
