"""GPU: the change report of tad_state_merge_changes / tad_state_replace_changes against the host model (tests/alerts_model.py): the
per-key array, the four counters, the call's own counters and the whole exported state after every call; no engine call on the reference
side.

Tables.  As tests/test_gpu_state_replace.py: point i of every key at T0 + 2 i, so that element indices and times translate and the odd
seconds are free for inserted points.  Every edge is asserted from host-side numbers — which element changes, which key_since that
gives — before the engine is asked.  Every case runs with the report in host memory, in device memory and as counters alone, on clones
of one loaded state."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadError, _capi
from theia_amd.engine import DeviceArray

import alerts_model as am
import replace_model as rm
import state_model as sm
from alerts_model import NO_CHANGE
from state_drivers import FIVE, T0, big, clone, execute_any, table_of
from state_helpers import HIST, SER, TIMES, assert_counts, assert_same, new_state, snapshot

pytestmark = pytest.mark.gpu

U64, I64 = np.uint64, np.int64
MODES = ("host", "device", "counters")


def loaded(engine, lens, flags, op, rng):
    rows = table_of(lens, rng, flags)
    st = new_state(engine, len(lens), flags)
    model = am.AlertsModel(len(lens), flags, op, 0.0)
    if rows[0].size:
        engine.run_stream(st, *rows, value_op=op)
        model.append(*rows)
    return st, model


def fresh(engine, st, model, flags):
    s2, m2 = clone(engine, st, model, flags)
    m = am.AlertsModel(m2.num_keys, m2.flags, m2.op, m2.alpha)
    m._set(*m2.points())
    return s2, m


def assert_report(got, want, mode, tag):
    """the report the stats dict carries against the model's"""
    for f in am.COUNTERS:
        assert got[f] == want[f], (tag, mode, f, got[f], want[f])
    assert got["keys_changed"] <= got["keys_touched"], (tag, mode, got["keys_changed"], got["keys_touched"])
    if mode == "counters":
        assert got["key_since"] is None, (tag, mode)
        return
    arr = got["key_since"].to_host() if isinstance(got["key_since"], DeviceArray) else got["key_since"]
    assert arr.dtype == I64 and arr.shape == want["key_since"].shape, (tag, mode, arr.dtype, arr.shape)
    bad = np.flatnonzero(arr != want["key_since"])
    assert bad.size == 0, (tag, mode, "key_since differs at keys", bad[:8].tolist(), arr[bad[:8]].tolist(), want["key_since"][bad[:8]].tolist())


def call(engine, st, model, kind, rows, mode, tag, expect=None, **kw):
    """one merge or replace with a report on the state and on the model: the model's report meets the host's own numbers (`expect`:
    key -> key_since, every other key NO_CHANGE; or a dict of counters) BEFORE the engine runs; then the stats, the report, the state"""
    k, t, v = (np.asarray(a) for a in rows)
    want = model.merge(k, t, v, **kw) if kind == "merge" else model.replace(k, t, v, **kw)
    rep = want.pop("changes")
    if expect is not None:
        since = np.full(model.num_keys, NO_CHANGE, I64)
        for key, s in expect.items():
            if isinstance(key, str):
                assert rep[key] == s, (tag, "host", key, rep[key], s)
            else:
                since[key] = s
        if any(not isinstance(key, str) for key in expect) or not expect:
            assert np.array_equal(rep["key_since"], since), (tag, "host", rep["key_since"].tolist()[:16], since.tolist()[:16])
    if kind == "merge":
        got = engine.merge_stream_changes(st, k, t, v, mode, value_op=model.op, **kw)
    else:
        got = engine.replace_stream_changes(st, k, t, v, mode, value_op=model.op, **kw)
    assert_counts(got, want, tag)
    assert_report(got, rep, mode, tag)
    assert_same(snapshot(st), model.expected_snapshot(), (tag, mode))
    return got, rep


FLAGS = (SER | TIMES, HIST | SER | TIMES)


@pytest.mark.parametrize("mode", MODES)
def test_what_does_not_change_a_key(engine, mode):
    """a sum of 0, a maximum not above the held value and a replace by the held value: combined / replaced points, touched and replayed
    keys, and no changed key; one differing value among them is the only change"""
    rng = np.random.default_rng(1)
    lens = [5, 0, 70, 3]
    for flags in FLAGS:
        for op in ("sum", "max"):
            st, m = loaded(engine, lens, flags, op, rng)
            wk, wt, wv = (a.copy() for a in m.points())
            sel = np.array([0, 2, 4, 5, 40, 74, 75, 77])               # elements of keys 0, 2 and 3
            same = wv[sel] if op == "max" else np.zeros(sel.size, U64)
            below = np.where(wv[sel] > 1, wv[sel] - U64(1), wv[sel]) if op == "max" else same
            for vals, what in ((same, "equal / zero"), (below, "below / zero")):
                got, _ = call(engine, st, m, "merge", (wk[sel], wt[sel], vals), mode, (flags, op, what), expect={"keys_changed": 0, "points_changed": 0})
                assert got["points_combined"] == sel.size and got["keys_touched"] == 3 and got["keys_replayed"] == 3
            got, _ = call(engine, st, m, "replace", (wk[sel], wt[sel], wv[sel]), mode, (flags, op, "replace by the held value"), expect={})
            assert got["points_replaced"] == sel.size and got["keys_touched"] == 3
            # one value of key 2 differs: element 40 - 5 = 35 of key 2
            vals = wv[sel].copy()
            vals[4] = vals[4] + U64(1)
            call(engine, st, m, "replace", (wk[sel], wt[sel], vals), mode, (flags, op, "one value differs"),
                 expect={2: T0 + 2 * 35, "points_changed": 1, "min_t": T0 + 2 * 35, "max_t": T0 + 2 * 35})
            inc = np.ones(sel.size, U64) if op == "sum" else wv[sel] + U64(3)
            call(engine, st, m, "merge", (wk[sel], wt[sel], inc), mode, (flags, op, "every value differs"),
                 expect={0: T0, 2: T0, 3: T0, "points_changed": sel.size, "min_t": T0, "max_t": T0 + 2 * 69})
            st.close()


@pytest.mark.parametrize("mode", MODES)
def test_the_same_ranged_reread_twice_reports_nothing_the_second_time(engine, mode):
    rng = np.random.default_rng(2)
    lens = [30, 0, 30, 12, 30]
    for flags in FLAGS:
        st, m = loaded(engine, lens, flags, "sum", rng)
        wk, wt, wv = (a.copy() for a in m.points())
        # the re-read of [T0 + 40, ..): keys 0 and 2 as held, key 4 with element 25 missing and a new point at T0 + 61, key 3 untouched
        sel = (wt >= T0 + 40) & ~((wk == 4) & (wt == T0 + 50))
        k, t, v = np.append(wk[sel], U64(4)), np.append(wt[sel], T0 + 61), np.append(wv[sel], FIVE[0])
        o = rng.permutation(k.size)
        rows = (k[o], t[o], v[o])
        kw = {"from_t": T0 + 40, "to_t": 0, "ranged": True}
        got, _ = call(engine, st, m, "replace", rows, mode, (flags, "first"), expect={4: T0 + 50, "points_changed": 2, "max_t": T0 + 61}, **kw)
        assert got["points_erased"] == 1 and got["points_appended"] == 1 and got["keys_touched"] == 3
        again, rep = call(engine, st, m, "replace", rows, mode, (flags, "second"), expect={}, **kw)
        assert again["keys_changed"] == 0 and again["points_changed"] == 0 and again["min_t"] == again["max_t"] == 0
        assert again["keys_touched"] == 3 and again["points_replaced"] == again["batch_points"]
        st.close()


@pytest.mark.parametrize("mode", MODES)
def test_erased_keys_outside_the_batch_and_emptied_keys(engine, mode):
    """a range erases on every key: a key changed only by an erase (no batch point), keys the batch names and keys it empties"""
    rng = np.random.default_rng(3)
    lens = [10, 4, 0, 10, 1, 2049]
    for flags in FLAGS:
        st0, m0 = loaded(engine, lens, flags, "sum", rng)
        none = sm._empty()
        # elements [3, 8) of every key: keys 0, 3, 5 lose five, key 1 loses its element 3, keys 2 and 4 nothing
        st, m = fresh(engine, st0, m0, flags)
        got, _ = call(engine, st, m, "replace", none, mode, (flags, "erase alone"), from_t=T0 + 6, to_t=T0 + 16, ranged=True,
                      expect={0: T0 + 6, 1: T0 + 6, 3: T0 + 6, 5: T0 + 6, "points_changed": 16, "min_t": T0 + 6, "max_t": T0 + 14})
        assert got["points_erased"] == 16 and got["keys_emptied"] == 0
        st.close()
        # everything from element 0 on, the batch names key 3's element 2 with its held value: keys 0, 1, 4, 5 emptied, key 3 keeps one
        st, m = fresh(engine, st0, m0, flags)
        wk, wt, wv = m.points()
        i = int(np.flatnonzero((wk == 3) & (wt == T0 + 4))[0])
        got, _ = call(engine, st, m, "replace", (wk[i:i + 1], wt[i:i + 1], wv[i:i + 1]), mode, (flags, "emptied"), from_t=0, to_t=0, ranged=True,
                      expect={0: T0, 1: T0, 3: T0, 4: T0, 5: T0, "points_changed": sum(lens) - 1, "max_t": T0 + 2 * 2048})
        assert got["keys_emptied"] == 4 and got["points_replaced"] == 1
        # the emptied keys refilled: the append path
        rows = (np.array([0, 4, 4], U64), np.array([T0 + 100, T0 + 3, T0 + 7], I64), big(rng, 3))
        got, _ = call(engine, st, m, "merge", rows, mode, (flags, "refill"), expect={0: T0 + 100, 4: T0 + 3, "points_changed": 3, "min_t": T0 + 3, "max_t": T0 + 100})
        assert got["keys_replayed"] == 0 and got["points_appended"] == 3
        st.close()
        # a range behind every point with a batch inside it: nothing erased, the batch appended
        st, m = fresh(engine, st0, m0, flags)
        last = T0 + 2 * 2048
        rows = (np.array([2, 5], U64), np.array([last + 10, last + 12], I64), big(rng, 2))
        got, _ = call(engine, st, m, "replace", rows, mode, (flags, "beyond"), from_t=last + 1, to_t=last + 100, ranged=True,
                      expect={2: last + 10, 5: last + 12, "points_changed": 2})
        assert got["keys_replayed"] == 0
        st.close()
        st0.close()


@pytest.mark.parametrize("mode", MODES)
def test_too_old_only_empty_and_in_order_batches(engine, mode):
    rng = np.random.default_rng(4)
    lens = [6, 0, 6, 1]
    for flags in FLAGS:
        st, m = loaded(engine, lens, flags, "sum", rng)
        snap = snapshot(st)
        rows = (np.array([0, 1, 2], U64), np.array([T0 + 1, T0 + 1, T0 + 2], I64), big(rng, 3))
        for kind in ("merge", "replace"):
            got, _ = call(engine, st, m, kind, rows, mode, (flags, kind, "all too old"), keep_from=T0 + 50, expect={"keys_changed": 0, "points_changed": 0})
            assert got["points_too_old"] == 3 and got["keys_touched"] == 0
            got, _ = call(engine, st, m, kind, sm._empty(), mode, (flags, kind, "empty"), expect={})
            assert got["batch_points"] == 0 and got["min_t"] == got["max_t"] == 0
        assert_same(snapshot(st), snap, "untouched")
        # the append path: every point newer than its key's last one (key 1 had none)
        rows = (np.array([0, 0, 1, 3, 3, 3], U64), np.array([T0 + 12, T0 + 30, T0 + 5, T0 + 2, T0 + 3, T0 + 9], I64), big(rng, 6))
        for kind in ("merge", "replace"):
            rows = (rows[0], rows[1] + 100, rows[2])
            o = rng.permutation(6)
            got, _ = call(engine, st, m, kind, tuple(a[o] for a in rows), mode, (flags, kind, "append path"),
                          expect={0: int(rows[1][0]), 1: int(rows[1][2]), 3: int(rows[1][3]), "points_changed": 6, "keys_changed": 3,
                                  "min_t": int(rows[1][3]), "max_t": int(rows[1][1])})
            assert got["keys_replayed"] == 0 and got["points_appended"] == 6 and got["keys_touched"] == 3
        # one too-old point sends an in-order batch through the full rewrite: the report is the same kind of report
        rows = (np.array([0, 2, 2], U64), np.array([T0 + 1, T0 + 500, T0 + 501], I64), big(rng, 3))
        got, _ = call(engine, st, m, "merge", rows, mode, (flags, "too old + newer"), keep_from=T0 + 3, expect={2: T0 + 500, "points_changed": 2, "max_t": T0 + 501})
        assert got["points_too_old"] == 1 and got["points_appended"] == 2
        st.close()


@pytest.mark.parametrize("at", (2047, 2048, 2049))
@pytest.mark.parametrize("mode", ("host", "device"))
def test_the_only_changed_point_of_a_4097_point_key_at_the_chunk_edge(engine, mode, at):
    """the key's [old | batch] elements are walked in chunks of 2048: equal-valued hits fill the first chunk before the one point that
    differs at element `at`, so that a chunk without a change must leave the key's entry alone and the right chunk must lower it"""
    rng = np.random.default_rng(5)
    lens = [3, 4097, 2]
    for flags in FLAGS:
        for kind, op in (("replace", "sum"), ("merge", "max"), ("merge", "sum")):
            st, m = loaded(engine, lens, flags, op, rng)
            wk, wt, wv = (a.copy() for a in m.points())
            mine = np.flatnonzero(wk == 1)
            sel = mine[np.r_[0:at + 1:1]]                                  # elements 0 .. at of key 1: `at` equal-valued hits, then the change
            vals = wv[sel].copy() if (kind, op) != ("merge", "sum") else np.zeros(sel.size, U64)
            vals[-1] = wv[sel[-1]] + U64(1) if (kind, op) != ("merge", "sum") else U64(1)
            t_at = T0 + 2 * at
            got, _ = call(engine, st, m, kind, (wk[sel], wt[sel], vals), mode, (flags, kind, op, at),
                          expect={1: t_at, "points_changed": 1, "keys_changed": 1, "min_t": t_at, "max_t": t_at})
            assert got["points_combined" if kind == "merge" else "points_replaced"] == at + 1
            # and the change alone, with an erase on the neighbours in a chunk of their own
            if kind == "replace":
                rows = (wk[sel[-1:]], wt[sel[-1:]], vals[-1:] + U64(1))
                call(engine, st, m, kind, rows, mode, (flags, "ranged", at), from_t=t_at - 2, to_t=t_at + 4, ranged=True,
                     expect={1: t_at - 2, "points_changed": 3, "min_t": t_at - 2, "max_t": t_at + 2})
            st.close()


LENS = (0, 1, 2047, 2048, 2049)


@pytest.mark.parametrize("mode", MODES)
def test_keys_of_every_length_around_the_chunk(engine, mode):
    """every key gets an inserted point before its last element, a combined point at its last element and an appended point: the batch's
    elements follow the old ones in the chunk walk, so the lengths put them in the first chunk, at its end and in a second one"""
    rng = np.random.default_rng(6)
    for flags in FLAGS:
        for kind, op in (("merge", "sum"), ("merge", "max"), ("replace", "sum")):
            st, m = loaded(engine, LENS, flags, op, rng)
            bk, bt, want = [], [], {}
            for j, n in enumerate(LENS):
                times = [T0 + 2 * n + 7] if n == 0 else [T0 + 2 * (n - 1) - 1, T0 + 2 * (n - 1), T0 + 2 * n + 7]
                bk += [j] * len(times)
                bt += times
                want[j] = times[0]
            bk, bt = np.array(bk, U64), np.array(bt, I64)
            vals = np.full(bk.size, (1 << 62) + 5, U64)                    # above every held value: a maximum takes it
            o = rng.permutation(bk.size)
            want.update(points_changed=int(bk.size), keys_changed=len(LENS), min_t=T0 - 1, max_t=T0 + 2 * 2049 + 7)   # (the one-point key's inserted point)
            got, _ = call(engine, st, m, kind, (bk[o], bt[o], vals[o]), mode, (flags, kind, op), expect=want)
            assert got["points_inserted"] == 4 and got["points_appended"] == 5
            st.close()


@pytest.mark.parametrize("K", (1, 63, 64, 65, 257))
def test_key_counts_around_the_wavefront(engine, K):
    """one lane per key in the report's passes: every third key changes (the last key always), on the rewrite path and on the append path"""
    rng = np.random.default_rng(7)
    flags = SER | TIMES
    lens = [4 + j % 3 for j in range(K)]
    for mode in MODES:
        st, m = loaded(engine, lens, flags, "sum", rng)
        keys = sorted(set(range(0, K, 3)) | {K - 1})
        rows = (np.array(keys, U64), np.full(len(keys), T0 + 3, I64), big(rng, len(keys)))
        got, _ = call(engine, st, m, "merge", rows, mode, (K, "inserted"), expect=dict({j: T0 + 3 for j in keys}, keys_changed=len(keys), points_changed=len(keys)))
        assert got["points_inserted"] == len(keys)
        rows = (np.array(keys, U64), np.array([T0 + 100 + j for j in keys], I64), big(rng, len(keys)))
        got, _ = call(engine, st, m, "replace", rows, mode, (K, "appended"),
                      expect=dict({j: T0 + 100 + j for j in keys}, keys_changed=len(keys), min_t=T0 + 100, max_t=T0 + 100 + K - 1))
        assert got["keys_replayed"] == 0
        got, _ = call(engine, st, m, "replace", sm._empty(), mode, (K, "erase all"), ranged=True, expect=dict({j: T0 for j in range(K)}, keys_changed=K))
        assert got["keys_emptied"] == K
        st.close()


def test_refusals_and_a_failed_call_leave_the_state_as_it_was(engine):
    rng = np.random.default_rng(8)
    flags = HIST | SER | TIMES
    K = 20
    st, m = loaded(engine, [8] * K, flags, "sum", rng)
    snap = snapshot(st)
    n = 60
    k, t, v = rng.integers(0, K, size=n).astype(U64), T0 + rng.integers(0, 40, size=n), big(rng, n)
    cols = _capi.Columns(n_rows=n, key_id=k.ctypes.data, flow_end_s=t.ctypes.data, value=v.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
    job = _capi.Job(algo=0, value_op=_capi.TAD_OP["sum"])
    lib, inv = engine._lib, _capi.TAD_ERR_INVALID_ARGUMENT
    arr = np.full(K + 1, 77, I64)
    bad = [_capi.Changes(key_since=arr.ctypes.data, len=K + 1, memory=0), _capi.Changes(key_since=arr.ctypes.data, len=K - 1, memory=0),
           _capi.Changes(key_since=arr.ctypes.data, len=0, memory=0), _capi.Changes(key_since=None, len=K, memory=0),
           _capi.Changes(key_since=arr.ctypes.data, len=K, memory=2), _capi.Changes(key_since=arr.ctypes.data + 4, len=K, memory=0)]
    for i, ch in enumerate(bad):
        ch.keys_changed = ch.points_changed = 9
        assert lib.tad_state_merge_changes(engine._h, st._h, C.byref(job), C.byref(cols), 0, None, C.byref(ch)) == inv, i
        assert ch.keys_changed == ch.points_changed == 0, i
        assert lib.tad_state_replace_changes(engine._h, st._h, C.byref(job), C.byref(cols), 1, 0, 0, 0, None, C.byref(ch)) == inv, i
        assert_same(snapshot(st), snap, ("refused report", i))
    assert (arr == 77).all()
    # a key out of range in the last row, with a report: TAD_ERR_KEY_RANGE, counters 0, the state as it was
    badk = k.copy()
    badk[-1] = K + 3
    for mode in MODES:
        for kw in ({}, {"ranged": True, "from_t": T0, "to_t": T0 + 30}):
            with pytest.raises(TadError) as ei:
                engine.replace_stream_changes(st, badk, t, v, mode, value_op="sum", **kw)
            assert ei.value.code == _capi.TAD_ERR_KEY_RANGE
        with pytest.raises(TadError) as ei:
            engine.merge_stream_changes(st, badk, t, v, mode, value_op="sum")
        assert ei.value.code == _capi.TAD_ERR_KEY_RANGE
        assert_same(snapshot(st), snap, ("key range", mode))
    ch = _capi.Changes(key_since=arr.ctypes.data, len=K, memory=0, keys_changed=5, points_changed=5, min_t=5, max_t=5)
    bcols = _capi.Columns(n_rows=n, key_id=badk.ctypes.data, flow_end_s=t.ctypes.data, value=v.ctypes.data, num_keys=K, memory=_capi.TAD_MEM_HOST)
    assert lib.tad_state_merge_changes(engine._h, st._h, C.byref(job), C.byref(bcols), 0, None, C.byref(ch)) == _capi.TAD_ERR_KEY_RANGE
    assert (ch.keys_changed, ch.points_changed, ch.min_t, ch.max_t) == (0, 0, 0, 0)
    # a NULL report is the old call; and the state still merges with a report after all that
    ms = _capi.MergeStats()
    assert lib.tad_state_merge_changes(engine._h, st._h, C.byref(job), C.byref(cols), 0, C.byref(ms), None) == 0
    want = m.merge(k, t, v)
    assert ms.points_combined == want["points_combined"] and ms.points_inserted == want["points_inserted"]
    call(engine, st, m, "replace", (k, t, v), "host", "after the refusals", from_t=T0, to_t=T0 + 9, ranged=True)
    st.close()


def test_the_feature_bit_is_set(engine):
    assert engine._lib.tad_features() & _capi.TAD_FEATURE_STATE_ALERTS


@pytest.mark.parametrize("seed", rm.SEEDS)
def test_every_merge_and_replace_of_the_seeded_scripts(engine, seed):
    """replace_model.make_script's eight scripts: every merge and replace runs with a report (host and device arrays in turn) and is
    compared with the diff of the model's table before and after it; the other operations run as the script says"""
    sc = rm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = rm.ReplaceModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    seen = 0
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], sm.describe(op))
        if op["kind"] not in ("merge", "replace"):
            st, _ = execute_any(engine, st, sc, op)
            rm.apply(model, op, rows=False)
            continue
        mode = MODES[seen % 2]
        seen += 1
        want, rep = am.apply_with_changes(model, op)
        k, t, v = op["k"], op["t"], op["v"]
        if op["cols"] == "host4":
            k, t = k.astype(np.uint32), t.astype(np.uint32)
        elif op["cols"] == "device":
            k, t, v = (DeviceArray.from_host(engine, a) for a in (k, t, v))
        with engine.plan(**op["plan"]):
            if op["kind"] == "merge":
                got = engine.merge_stream_changes(st, k, t, v, mode, value_op=sc["op"], alpha=sc["alpha"], keep_from=op["keep_from"])
            else:
                got = engine.replace_stream_changes(st, k, t, v, mode, from_t=op["from_t"], to_t=op["to_t"], ranged=op["ranged"], value_op=sc["op"],
                                                    alpha=sc["alpha"], keep_from=op["keep_from"])
        assert_counts(got, want["stats"], tag)
        assert_report(got, rep, mode, tag)
        assert_same(snapshot(st), model.expected_snapshot(), (tag, "state"))
    assert seen >= 2, (seed, seen)
    st.close()
