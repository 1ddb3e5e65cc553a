"""GPU: tad_state_replace against the host model (tests/replace_model.py): the whole exported state — moments, series, times, history —
bit for bit, and the call's counters, after every call; no engine call on the reference side.

Values.  sum: every value carries 50 to 62 significant bits, so that a value combined instead of replaced, or a replay in another order,
shows in the low bits.  max: the batch's values are smaller than the ones they replace, so that max(old, new) instead of new shows.
Where a history is kept the values come from a set of five, so that erased, replaced and kept values tie in the sorted history.

Times.  The edge tables keep point i of every key at T0 + 2 i: a range [T0 + 2 x, T0 + 2 y) erases the elements [x, y) of every key, both
bounds exactly on a point's second, and the odd seconds are free for inserted points.  Every edge is asserted from host-side numbers —
the element indices of the run, the counters the model gives — before the engine is asked, and every edge call is made twice."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadError, _capi
from theia_amd.engine import DeviceArray

import replace_model as rm
import state_model as sm
from state_drivers import T0, big, clone, execute_any, old_values, run_check, table_of
from state_helpers import HIST, SER, TIMES, assert_counts, assert_rows, assert_same, bits, new_state, rows_of, snapshot

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
LENS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097)
FIVE_SMALL = np.array([3, 1 << 20, 77, (1 << 33) + 5, 12], U64)      # below every value of FIVE: what a max must not keep


def new_values(rng, n, flags, op):
    if op == "max":
        return FIVE_SMALL[rng.integers(0, 5, size=n)] if flags & HIST else rng.integers(1, 1 << 40, size=n).astype(U64)
    return old_values(rng, n, flags)


def loaded(engine, lens, flags, op, rng, alpha=0.0):
    """-> (state, model) holding table_of(lens): one stream batch on the state, the same rows into the model"""
    rows = table_of(lens, rng, flags)
    st = new_state(engine, len(lens), flags)
    model = rm.ReplaceModel(len(lens), flags, op, alpha)
    if rows[0].size:
        engine.run_stream(st, *rows, value_op=op, alpha=alpha)
        model.append(*rows)
    assert_same(snapshot(st), model.expected_snapshot(), "loaded")
    return st, model


def replace(engine, st, model, rows, from_t=0, to_t=0, ranged=False, keep_from=0, expect=None, tag="", twice=True, device=False, narrow=False):
    """one tad_state_replace on the state and on the model: the counters the host expects (`expect`, asserted BEFORE the engine runs), the
    call's counters, the whole state; then the same call again: the same bits, nothing erased, inserted or appended"""
    k, t, v = (np.asarray(a) for a in rows)
    want = model.replace(k, t, v, from_t, to_t, ranged, keep_from)
    for f, x in (expect or {}).items():
        assert want[f] == x, (tag, "host", f, want[f], x)
    expected = model.expected_snapshot()

    def call():
        kk, tt, vv = (k.astype(np.uint32), t.astype(np.uint32), v) if narrow else (k, t, v)
        if device:
            kk, tt, vv = (DeviceArray.from_host(engine, a) for a in (kk, tt, vv))
        return engine.replace_stream(st, kk, tt, vv, from_t=from_t, to_t=to_t, ranged=ranged, value_op=model.op, alpha=model.alpha, keep_from=keep_from)

    got = call()
    assert_counts(got, want, (tag, "first call"))
    assert_same(snapshot(st), expected, (tag, "first call"))
    if twice:
        want2 = model.replace(k, t, v, from_t, to_t, ranged, keep_from)
        again = call()
        assert_counts(again, want2, (tag, "second call"))
        assert again["points_erased"] == again["points_inserted"] == again["points_appended"] == again["keys_emptied"] == 0, (tag, again)
        assert again["points_replaced"] == again["batch_points"] - again["points_too_old"], (tag, again)
        assert_same(snapshot(st), expected, (tag, "second call"))
    return got


def run_len(n, x, y):
    """elements of a key of n points inside the element run [x, y)"""
    return max(0, min(n, y) - min(n, x))


FLAGS_OPS = [(f, o) for f in (SER | TIMES, HIST | SER | TIMES) for o in ("sum", "max")]
IDS = ["flags%d-%s" % fo for fo in FLAGS_OPS]

# element runs [x, y): starting and ending at 0, 1, a - 1 and a of the keys of LENS, and around the chunk edge 2047 | 2048 | 2049
RUNS = [(0, 1), (1, 2), (0, 2), (1, 63), (62, 63), (63, 64), (63, 65), (64, 65), (2, 2047), (2046, 2047), (2047, 2048), (2047, 2049), (2048, 2049),
        (2040, 2060), (1, 2048), (2048, 4097), (4096, 4097), (0, 4097)]


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_runs_at_every_length_and_chunk_edge_without_a_batch_point(engine, flags, op):
    """the empty batch with R: every key loses exactly the elements [x, y) it has; no key has a batch point"""
    rng = np.random.default_rng(11)
    st0, m0 = loaded(engine, LENS, flags, op, rng)
    none = sm._empty()
    for x, y in RUNS:
        st, m = clone(engine, st0, m0, flags)
        erased = sum(run_len(n, x, y) for n in LENS)
        emptied = sum(1 for n in LENS if n and run_len(n, x, y) == n)
        got = replace(engine, st, m, none, T0 + 2 * x, T0 + 2 * y, True, tag=(x, y),
                      expect={"points_erased": erased, "keys_emptied": emptied, "batch_points": 0})
        assert got["keys_replayed"] == sum(1 for n in LENS if run_len(n, x, y)), (x, y, got)
        st.close()
    st0.close()


def edge_batch(rng, flags, op, x, y, keys):
    """for every key of `keys` (index, length): a replaced point at the first and at the last element of the run, an inserted point at the
    odd second inside the run, one before it and one behind it, and an appended point — whatever of those the key's length allows"""
    bk, bt = [], []
    for j, n in keys:
        idx = set()
        if x < n:
            idx.add(2 * x)                       # replaced: the run's first element
            idx.add(2 * (min(y, n) - 1))         # replaced: its last one
            idx.add(2 * x + 1)                   # inserted inside the run (or appended, when the run ends the key)
        if x > 0:
            idx.add(2 * min(x, n) - 1)           # inserted just before the run (appended behind a shorter key)
        idx.add(2 * y + 1)                       # behind the run: inserted, or appended behind an erased tail
        idx.add(2 * max(n, y) + 5)               # appended
        for i in sorted(idx):
            bk.append(j)
            bt.append(T0 + i)
    bk, bt = np.array(bk, U64), np.array(bt, I64)
    o = rng.permutation(bk.size)
    return bk[o], bt[o], new_values(rng, bk.size, flags, op)


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_runs_with_replaced_inserted_and_appended_points_on_some_keys(engine, flags, op):
    """keys 3, 6 and 9 (63, 2047 and 4097 points) get batch points at the run's first and last element, inside, before and behind it;
    the other keys have erased points and no batch point, in the same wavefront of the per-key kernels"""
    rng = np.random.default_rng(12)
    st0, m0 = loaded(engine, LENS, flags, op, rng)
    with_batch = [(3, LENS[3]), (6, LENS[6]), (9, LENS[9])]
    for x, y in RUNS:
        st, m = clone(engine, st0, m0, flags)
        rows = edge_batch(rng, flags, op, x, y, with_batch)
        # host side: the replaced points are the even seconds below 2 n, and they are not erased
        rep = int(sum(1 for j, s in zip(rows[0].tolist(), rows[1].tolist()) if (s - T0) % 2 == 0 and (s - T0) // 2 < LENS[j]))
        in_run_rep = int(sum(1 for j, s in zip(rows[0].tolist(), rows[1].tolist()) if (s - T0) % 2 == 0 and x <= (s - T0) // 2 < min(y, LENS[j])))
        assert rep == in_run_rep and rep >= 1
        erased = sum(run_len(n, x, y) for n in LENS) - rep
        got = replace(engine, st, m, rows, T0 + 2 * x, T0 + 2 * y, True, tag=(x, y),
                      expect={"points_replaced": rep, "points_erased": erased, "points_too_old": 0})
        assert got["points_appended"] >= 3 and got["points_inserted"] + got["points_appended"] + rep == got["batch_points"], (x, y, got)
        st.close()
    st0.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_bounds_between_points_open_sides_and_degenerate_ranges(engine, flags, op):
    rng = np.random.default_rng(13)
    st0, m0 = loaded(engine, LENS, flags, op, rng)
    total = sum(LENS)
    last = T0 + 2 * (max(LENS) - 1)
    batch = (np.array([5, 9, 9], U64), np.array([T0 + 40, T0 + 41, T0 + 100], I64), new_values(rng, 3, flags, op))
    cases = [
        # (from_t, to_t, ranged, erased without a batch, what)
        (T0 + 2 * 10 - 1, T0 + 2 * 20 - 1, True, sum(run_len(n, 10, 20) for n in LENS), "both bounds between two points"),
        (T0 + 2 * 10, T0 + 2 * 10 + 1, True, sum(run_len(n, 10, 11) for n in LENS), "one second wide, on a point"),
        (T0 + 2 * 10 + 1, T0 + 2 * 10 + 2, True, 0, "one second wide, between points"),
        (T0 + 2 * 10, T0 + 2 * 10, True, 0, "from_t == to_t"),
        (last + 1, last + 1000, True, 0, "beyond every time"),
        (1, T0, True, 0, "before every time"),
        (0, 0, True, total, "everything"),
        (T0 + 2 * 64, 0, True, sum(run_len(n, 64, n) for n in LENS), "from_t alone"),
        (0, T0 + 2 * 64, True, sum(run_len(n, 0, 64) for n in LENS), "to_t alone"),
        (0, last, True, total - 1, "to_t on the newest point: it stays"),
        (T0, last + 1, True, total, "from the oldest second to behind the newest"),
        (0, 0, False, 0, "no range"),
    ]
    for from_t, to_t, ranged, erased, what in cases:
        st, m = clone(engine, st0, m0, flags)
        replace(engine, st, m, sm._empty(), from_t, to_t, ranged, tag=what, expect={"points_erased": erased})
        st.close()
        st, m = clone(engine, st0, m0, flags)      # the same range with a batch of three points: key 5 replaced at 40, key 9 inserted at 41, replaced at 100
        in_r = rm.in_range(batch[1], from_t, to_t, ranged)
        replace(engine, st, m, batch, from_t, to_t, ranged, tag=(what, "batch"),
                expect={"points_erased": erased - int((in_r & (batch[1] % 2 == 0)).sum()), "points_replaced": 2, "points_inserted": 1})
        st.close()
    st0.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_a_key_with_erased_points_and_no_batch_point_alone_and_among_64(engine, flags, op):
    rng = np.random.default_rng(14)
    # alone in its wavefront: a state of one key
    st, m = loaded(engine, [300], flags, op, rng)
    replace(engine, st, m, sm._empty(), T0 + 2 * 100, T0 + 2 * 200, True, tag="one key", expect={"points_erased": 100, "keys_emptied": 0})
    st.close()
    # among 64 (and past the first wavefront of keys): 130 keys of 5 points, key 70 alone reaches into the range; its neighbours have batch points
    lens = [5] * 130
    lens[70] = 40
    st, m = loaded(engine, lens, flags, op, rng)
    bk = np.array([69, 71, 0, 129], U64)
    rows = (bk, np.array([T0 + 4, T0 + 5, T0 + 2 * 30, T0 + 3], I64), new_values(rng, 4, flags, op))
    got = replace(engine, st, m, rows, T0 + 2 * 10, T0 + 2 * 35, True, tag="among 64",
                  expect={"points_erased": 25, "points_replaced": 1, "points_inserted": 2, "points_appended": 1, "keys_emptied": 0})
    assert got["keys_replayed"] == 4 and got["keys_touched"] == 5, got
    # every key of all three wavefronts of keys loses its elements 3 and 4, none has a batch point
    replace(engine, st, m, sm._empty(), T0 + 2 * 3, T0 + 2 * 5, True, tag="all keys", expect={"points_erased": 2 * 130, "keys_emptied": 0})
    st.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_chunks_of_2048_and_2049_elements_with_the_run_across_the_edge(engine, flags, op):
    """the series kernel walks [old points | batch points] in chunks of 2048: a + b = 2048 (one wavefront) and 2049 (a second one for the
    last batch point), the erased run reaching over the last old elements and the batch points replacing, inserting and appending in it"""
    rng = np.random.default_rng(15)
    for b in (8, 9):
        a = 2040
        st, m = loaded(engine, [a, 7], flags, op, rng)
        # b points on key 0: replaced at elements 2030 and 2039, inserted at the odd seconds behind 2031.., appended behind the end
        secs = [2 * 2030, 2 * 2039, 2 * 2031 + 1, 2 * 2033 + 1, 2 * 2038 + 1, 2 * a + 1, 2 * a + 3, 2 * a + 9][:8] + ([2 * a + 11] if b == 9 else [])
        assert a + len(secs) == 2040 + b
        rows = (np.zeros(len(secs), U64), T0 + np.array(secs, I64), new_values(rng, len(secs), flags, op))
        o = rng.permutation(len(secs))
        rows = tuple(c[o] for c in rows)
        replace(engine, st, m, rows, T0 + 2 * 2025, T0 + 2 * a + 4, True, tag=("a + b", a + b),
                expect={"points_replaced": 2, "points_inserted": 3, "points_appended": b - 5, "points_erased": 15 - 2, "keys_emptied": 0})
        st.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_the_unranged_replace_at_the_chunk_edges(engine, flags, op):
    """without TAD_REPLACE_RANGE the series kernel runs with the replace rule and no range code: the batches of the ranged edge tests —
    replaced, inserted and appended points on both sides of every 2048-element chunk edge of keys 3, 6 and 9 — with nothing erased"""
    rng = np.random.default_rng(18)
    st0, m0 = loaded(engine, LENS, flags, op, rng)
    with_batch = [(3, LENS[3]), (6, LENS[6]), (9, LENS[9])]
    for x, y in RUNS:
        st, m = clone(engine, st0, m0, flags)
        rows = edge_batch(rng, flags, op, x, y, with_batch)
        rep = int(sum(1 for j, s in zip(rows[0].tolist(), rows[1].tolist()) if (s - T0) % 2 == 0 and (s - T0) // 2 < LENS[j]))
        assert rep >= 1
        got = replace(engine, st, m, rows, 0, 0, False, tag=(x, y),
                      expect={"points_replaced": rep, "points_erased": 0, "keys_emptied": 0, "points_too_old": 0})
        assert got["points_appended"] >= 3 and got["points_inserted"] + got["points_appended"] + rep == got["batch_points"], (x, y, got)
        st.close()
    st0.close()
    # a + b = 2048 (one wavefront) and 2049 (a second one for the last batch point), as the ranged test has them
    for b in (8, 9):
        a = 2040
        st, m = loaded(engine, [a, 7], flags, op, rng)
        secs = [2 * 2030, 2 * 2039, 2 * 2031 + 1, 2 * 2033 + 1, 2 * 2038 + 1, 2 * a + 1, 2 * a + 3, 2 * a + 9][:8] + ([2 * a + 11] if b == 9 else [])
        assert a + len(secs) == 2040 + b
        rows = (np.zeros(len(secs), U64), T0 + np.array(secs, I64), new_values(rng, len(secs), flags, op))
        o = rng.permutation(len(secs))
        rows = tuple(c[o] for c in rows)
        replace(engine, st, m, rows, 0, 0, False, tag=("a + b", a + b),
                expect={"points_replaced": 2, "points_inserted": 3, "points_appended": b - 5, "points_erased": 0, "keys_emptied": 0})
        st.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_keys_emptied_refilled_and_batches_outside_the_range(engine, flags, op):
    rng = np.random.default_rng(16)
    lens = [10, 10, 10, 10, 0, 3000]
    st0, m0 = loaded(engine, lens, flags, op, rng)
    end = T0 + 2 * 3000
    # a key emptied (0), a key emptied and refilled by the batch inside R (1) and behind R (2), a key with batch points outside R only (3),
    # an unseen key that gets its first points (4), a long key that keeps its tail (5)
    bk = np.array([1, 1, 2, 3, 3, 4, 4], U64)
    bt = np.array([T0 + 3, T0 + 4, end + 50, end + 60, end + 61, T0 + 1, end + 7], I64)
    rows = (bk, bt, new_values(rng, 7, flags, op))
    st, m = clone(engine, st0, m0, flags)
    got = replace(engine, st, m, rows, T0, T0 + 2 * 10, True, tag="emptied",
                  expect={"points_erased": 49, "points_replaced": 1, "points_inserted": 1, "points_appended": 5, "keys_emptied": 1})
    n = snapshot(st)["state"]["n"]
    assert n.tolist() == [0, 2, 1, 2, 2, 2990], n
    assert got["keys_replayed"] == 5, got            # keys 0, 1, 2, 3 (erased) and 5 (erased); key 4 only appended
    st.close()
    # a batch entirely too old: with R it still erases R, without R the state stays as it is
    st, m = clone(engine, st0, m0, flags)
    old = (np.array([0, 5, 5], U64), np.array([T0 + 2, T0 + 4, T0 + 5], I64), new_values(rng, 3, flags, op))
    replace(engine, st, m, old, 0, 0, False, keep_from=T0 + 1000, tag="too old, no R",
            expect={"points_too_old": 3, "points_erased": 0, "points_replaced": 0, "points_inserted": 0, "points_appended": 0})
    assert_same(snapshot(st), snapshot(st0), "too old, no R: unchanged")
    replace(engine, st, m, old, T0 + 2, T0 + 8, True, keep_from=T0 + 1000, tag="too old, R",
            expect={"points_too_old": 3, "points_erased": 3 * 5, "points_replaced": 0, "keys_emptied": 0})
    st.close()
    # R = everything and a batch: the state is a fresh state fed the batch
    st, m = clone(engine, st0, m0, flags)
    replace(engine, st, m, rows, 0, 0, True, tag="everything", expect={"points_erased": sum(lens) - 1, "keys_emptied": 2})
    fresh = rm.ReplaceModel(len(lens), flags, op, 0.0)
    fresh.append(*rows)
    assert_same(snapshot(st), fresh.expected_snapshot(), "everything == fresh")
    st.close()
    st0.close()


@pytest.mark.parametrize("flags,op", FLAGS_OPS, ids=IDS)
def test_the_in_order_batch_takes_the_append_path(engine, flags, op):
    rng = np.random.default_rng(17)
    lens = [20, 0, 300, 2048]
    st, m = loaded(engine, lens, flags, op, rng)
    end = T0 + 2 * 2048
    bk = np.array([0, 0, 1, 3, 3, 3], U64)
    bt = np.array([end + 1, end + 2, end + 1, end, end + 5, end + 9], I64)
    rows = (bk, bt, new_values(rng, 6, flags, op))
    for ranged, rng_ in ((False, (0, 0)), (True, (end, end + 100))):      # the poll loop's range holds nothing old: still the append path
        s2, m2 = clone(engine, st, m, flags)
        got = replace(engine, s2, m2, rows, rng_[0], rng_[1], ranged, tag=("in order", ranged), twice=False,
                      expect={"points_appended": 6, "points_inserted": 0, "points_replaced": 0, "points_erased": 0})
        assert got["keys_replayed"] == 0 and got["keys_touched"] == 3, got
        s2.close()
    # one erased point anywhere sends the same batch through the rewrite
    got = replace(engine, st, m, rows, end - 2, end + 100, True, tag="in order, one erased", expect={"points_appended": 6, "points_erased": 1})
    assert got["keys_replayed"] == 1, got
    st.close()


# ---- re-read polls ----
def poll_table():
    """about 20 000 points over 300 keys and 800 seconds, 1.3 rows per point, every row arriving up to 119 s late"""
    rng = np.random.default_rng(21)
    K, span, n = 300, 800, 20000
    pk = rng.integers(0, K, size=n).astype(U64)
    pt = T0 + rng.integers(0, span, size=n)
    twice = rng.random(n) < 0.3
    k, t = np.concatenate([pk, pk[twice]]), np.concatenate([pt, pt[twice]])
    return K, k, t, big(rng, k.size), t + rng.integers(0, 120, size=k.size)


POLL_LAG = 150


def polls():
    """-> [(from_t, to_t, rows)]: poll p at now = T0 + 100 (p + 1) (the last one late enough for every row) reads all rows that have arrived
    with flowEndSeconds in [watermark - lag, now), shuffled"""
    K, k, t, v, arrival = poll_table()
    rng = np.random.default_rng(22)
    out, wm = [], T0
    for p in range(8):
        now = T0 + 100 * (p + 1) + (POLL_LAG if p == 7 else 0)
        from_t = wm - POLL_LAG
        sel = np.flatnonzero((t >= from_t) & (t < now) & (arrival <= now))
        sel = sel[rng.permutation(sel.size)]
        out.append((from_t, now, (k[sel], t[sel], v[sel])))
        wm = now
    return K, (k, t, v), out


@pytest.mark.parametrize("flags", [SER | TIMES, HIST | SER | TIMES], ids=["flags10", "flags11"])
def test_overlapping_re_read_polls_leave_the_table_each_row_once(engine, flags):
    K, table, ps = polls()
    st = new_state(engine, K, flags)
    model = rm.ReplaceModel(K, flags, "sum", 0.0)
    seen_twice = 0
    for p, (from_t, to_t, rows) in enumerate(ps):
        got = replace(engine, st, model, rows, from_t, to_t, True, tag=("poll", p), twice=False, device=p % 2 == 1, narrow=p == 4)
        seen_twice += got["points_replaced"]
        assert p == 0 or got["points_replaced"] > 0, (p, got)
    assert seen_twice > 5000
    whole = rm.ReplaceModel(K, flags, "sum", 0.0)
    whole.append(*table)
    assert_same(snapshot(st), whole.expected_snapshot(), "all polls == one stream batch over the table")
    # the same polls through tad_state_merge double what they saw twice: this file can see the fault it is about
    twin = new_state(engine, K, flags)
    for from_t, to_t, rows in ps:
        engine.merge_stream(twin, *rows, value_op="sum")
    assert np.array_equal(twin.export_times(), st.export_times())
    assert not np.array_equal(twin.export_series()[1], st.export_series()[1])
    twin.close()
    st.close()


# ---- sequences ----


@pytest.mark.parametrize("seed", rm.SEEDS)
def test_sequence_with_replaces(engine, seed):
    sc = rm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = rm.ReplaceModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], sm.describe(op))
        st, got = execute_any(engine, st, sc, op)
        want = rm.apply(model, op)
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        if "raises" in want:
            assert got["raises"], (tag, "the call must be refused")
        if "rows" in want:
            assert_rows(got["rows"], want["rows"], (tag, "rows"))
        if op["kind"] in ("merge", "replace"):
            assert_counts(got["stats"], want["stats"], tag)
        if "dropped" in want:
            assert got["dropped"] == want["dropped"], (tag, got["dropped"], want["dropped"])
        if "remap" in want:
            assert np.array_equal(bits(got["remap"]), bits(want["remap"])), (tag, "remap")
        assert st.num_keys == model.num_keys, (tag, st.num_keys, model.num_keys)
        expected = model.expected_snapshot()
        assert_same(snapshot(st), expected, (tag, "state"))
        for check in op["checks"]:
            ctag = (tag, check["call"], check["algo"], check["emit_all"], check["params"], check.get("win"), check.get("mask_kind"))
            res = run_check(engine, st, check)
            rows, counters = model.check_expect(check)
            assert_rows(rows_of(res), rows, ctag)
            for f, x in counters.items():
                assert res.stats[f] == x, (ctag, f, res.stats[f], x)
        assert_same(snapshot(st), expected, (tag, "state after the read-only jobs"))
    st.close()


# ---- after a replace ----
def test_jobs_and_stream_batches_after_a_replace(engine):
    """tad_run_state for EWMA, DBSCAN and a small ARIMA table == tad_run over W'; a later DBSCAN stream batch emits what the batch job over
    W' ++ batch emits for the batch's points"""
    rng = np.random.default_rng(31)
    flags = HIST | SER | TIMES
    K, per = 6, 30
    k = np.repeat(np.arange(K, dtype=U64), per)
    t = T0 + 60 * np.tile(np.arange(per, dtype=I64), K)
    v = (1_000_000 + rng.integers(0, 500_000, size=k.size)).astype(U64)
    st = new_state(engine, K, flags)
    model = rm.ReplaceModel(K, flags, "sum", 0.0)
    engine.run_stream(st, k, t, v, value_op="sum")
    model.append(k, t, v)
    sel = rng.random(k.size) < 0.4
    rows = (k[sel], t[sel], (2_000_000 + rng.integers(0, 9_000_000, size=int(sel.sum()))).astype(U64))
    replace(engine, st, model, rows, T0 + 60 * 10, T0 + 60 * 22, True, tag="before the jobs")
    wk, wt, wv = model.points()
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        for emit_all in (False, True):
            got = engine.run_state(st, algo=algo, emit_all=emit_all)
            want = engine.run(algo, wk, wt, wv, K, value_op="sum", emit_all=emit_all)
            assert_rows(rows_of(got), rows_of(want), (algo, emit_all))
            rows_m, _ = model.job(algo, emit_all=emit_all)
            assert_rows(rows_of(got), rows_m, (algo, emit_all, "model"))
    nk = np.repeat(np.arange(K, dtype=U64), 3)
    nt = T0 + 60 * (per + np.tile(np.arange(3, dtype=I64), K))
    nv = (1_000_000 + rng.integers(0, 30_000_000, size=nk.size)).astype(U64)
    for emit_all in (False, True):
        s2, m2 = clone(engine, st, model, flags)
        res = engine.run_stream(s2, nk, nt, nv, value_op="sum", algo="DBSCAN", emit_all=emit_all)
        pts = m2.append(nk, nt, nv)
        assert_rows(rows_of(res), m2.stream_rows(None, pts, "DBSCAN", emit_all, {}), ("stream DBSCAN", emit_all))
        assert_same(snapshot(s2), m2.expected_snapshot(), "after the stream batch")
        s2.close()
    st.close()


# ---- refusals and atomicity ----
def test_refusals_leave_the_state_unchanged(engine):
    rng = np.random.default_rng(41)
    flags = HIST | SER | TIMES
    K = 50
    st, model = loaded(engine, [20] * K, flags, "sum", rng)
    snap = snapshot(st)
    n = 200
    k, t, v = rng.integers(0, K, size=n).astype(U64), T0 + rng.integers(0, 60, size=n), big(rng, n)
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    bad = [({"from_t": T0 + 5}, "from_t without the flag"), ({"to_t": T0 + 5}, "to_t without the flag"),
           ({"from_t": T0 + 9, "to_t": T0 + 5, "ranged": True}, "from_t after to_t"),
           ({"num_keys": K + 1}, "num_keys"), ({"alpha": 1.5}, "alpha"), ({"alpha": -0.1}, "alpha")]
    for kw, what in bad:
        with pytest.raises(TadError) as ei:
            engine.replace_stream(st, k, t, v, value_op="sum", **kw)
        assert ei.value.code == inv, what
        assert ei.value.args and str(ei.value), what
        assert_same(snapshot(st), snap, what)
    # unknown flag bits and TAD_FLAG_EMIT_ALL_POINTS through the C call itself
    kk, tt, vv = np.ascontiguousarray(k), np.ascontiguousarray(t), np.ascontiguousarray(v)
    cols = _capi.Columns(n_rows=kk.size, key_id=kk.ctypes.data, flow_end_s=tt.ctypes.data, value=vv.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
    job = _capi.Job(algo=0, value_op=_capi.TAD_OP["sum"])
    rs = _capi.ReplaceStats()
    lib = engine._lib
    for fl in (2, 3, 0x80000000):
        assert lib.tad_state_replace(engine._h, st._h, C.byref(job), C.byref(cols), fl, 0, 0, 0, C.byref(rs)) == inv, fl
    emit = _capi.Job(algo=0, value_op=_capi.TAD_OP["sum"], flags=_capi.TAD_FLAG_EMIT_ALL_POINTS)
    assert lib.tad_state_replace(engine._h, st._h, C.byref(emit), C.byref(cols), 1, 0, 0, 0, C.byref(rs)) == inv
    assert lib.tad_state_replace(engine._h, st._h, C.byref(emit), C.byref(cols), 1, 0, 0, 0, None) == inv
    assert lib.tad_state_replace(engine._h, st._h, None, C.byref(cols), 1, 0, 0, 0, None) == inv
    nocol = _capi.Columns(n_rows=kk.size, key_id=kk.ctypes.data, flow_end_s=None, value=vv.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
    assert lib.tad_state_replace(engine._h, st._h, C.byref(job), C.byref(nocol), 1, 0, 0, 0, C.byref(rs)) == inv
    assert_same(snapshot(st), snap, "C refusals")
    # a key id out of range in the LAST row: everything before it was aggregated, nothing is committed
    badk = k.copy()
    badk[-1] = K + 3
    for kw in ({}, {"ranged": True, "from_t": T0, "to_t": T0 + 30}):
        with pytest.raises(TadError) as ei:
            engine.replace_stream(st, badk, t, v, value_op="sum", **kw)
        assert ei.value.code == _capi.TAD_ERR_KEY_RANGE
        assert_same(snapshot(st), snap, ("key range", kw))
    # states that cannot place a point by time, and stale times
    for fl in (0, HIST, SER, HIST | SER):
        other = new_state(engine, K, fl)
        engine.run_stream(other, k, t + 1000, v, value_op="sum")
        osnap = snapshot(other)
        with pytest.raises(TadError) as ei:
            engine.replace_stream(other, k, t, v, value_op="sum")
        assert ei.value.code == inv, fl
        assert_same(snapshot(other), osnap, fl)
        other.close()
    stale = new_state(engine, K)
    stale.load(snap["state"])
    stale.load_series(*snap["series"])
    with pytest.raises(TadError) as ei:
        engine.replace_stream(stale, k, t, v, value_op="sum")
    assert ei.value.code == inv
    stale.close()
    # a successful call without stats, and the state still replaces after all that
    assert lib.tad_state_replace(engine._h, st._h, C.byref(job), C.byref(cols), 1, T0, T0 + 30, 0, None) == 0
    model.replace(k, t, v, T0, T0 + 30, True)
    assert_same(snapshot(st), model.expected_snapshot(), "after the refusals")
    st.close()
