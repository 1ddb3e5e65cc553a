"""GPU: seeded sequences of operations on one streaming state against a host model of the whole state API (tests/state_model.py).

Every call on a state is defined by include/tad.h as a function of the table W of points the state holds, so the reference side is W
and the oracles alone: no engine call, no twin state.  A script (state_model.make_script) mixes stream batches of all four detectors,
refused late batches, merges (late, re-sent, in-order, with keep_from), trims, compactions, resizes, restarts through export / import
and calls that must be refused, over four shape classes; the columns are 8 or 4 bytes wide, on the host or the device, under the sparse
and both dense Stage 0.  After EVERY operation: the call's own outputs (rows, merge counters, points dropped, remap and compact
counters, num_keys) equal the model's; the whole state — moments, series, times, history — equals the model's expected snapshot; two
read-only jobs (run_state, and one of run_state_window / run_state_keys / drop_state / drop_state_keys over a drawn window and key
mask) return the oracle's rows and counters and leave the state as it was.  Everything is compared as bit patterns; there is no
tolerance in this file.

What the seed set covers is asserted on the host by tests/test_state_model.py.  A failure names (seed, operation index, kind,
arguments); replay(engine, seed, upto) below rebuilds the state as it was before operation `upto`.

Time.  The reference side was measured once per seed on one host core without a device: building the script, the model's steps, every
expected snapshot and every oracle job take at most 0.8 s of a seed (seeds 3, 28 and 29, the 700- and 3000-key states; 6.4 s for all
32), against a budget of 20 s per seed.  On an MI355X the 32 seeds take 5 s together, the slowest (seed 2, ARIMA) 0.45 s."""
import numpy as np
import pytest

from theia_amd import TadError
from theia_amd.engine import DeviceArray

import state_model as sm
from test_gpu_state_merge import assert_counts, new_state
from test_gpu_state_run import assert_rows, assert_same, bits, raw_run_state, rows_of, snapshot

pytestmark = pytest.mark.gpu

COMPACT_FIELDS = ("keys_before", "keys_after", "num_keys", "keys_unseen", "keys_idle", "points_dropped")


def columns(engine, op):
    """the batch's columns as the script drew them: 8-byte host arrays, 4-byte key and time columns, or device arrays"""
    k, t, v = op["k"], op["t"], op["v"]
    if op["cols"] == "host4":
        return k.astype(np.uint32), t.astype(np.uint32), v
    if op["cols"] == "device":
        return tuple(DeviceArray.from_host(engine, a) for a in (k, t, v))
    return k, t, v


def engine_params(algo, params):
    if algo == "DROP":
        return {"nsigma": params["nsigma"], "min_samples": params["drop_min_samples"]}
    return dict(params)


def stream_batch(engine, st, sc, op, algo, **kw):
    k, t, v = columns(engine, op)
    with engine.plan(**op["plan"]):
        if algo == "DROP":
            return engine.drop_stream(st, k, t, v, value_op=sc["op"], alpha=sc["alpha"], emit_all=op["emit_all"], **kw)
        return engine.run_stream(st, k, t, v, value_op=sc["op"], alpha=sc["alpha"], algo=algo, emit_all=op["emit_all"], **kw)


def restart(engine, st, flags):
    """export every part, a fresh state, import: the host restarted"""
    snap = snapshot(st)
    fresh = new_state(engine, st.num_keys, flags)
    fresh.load(snap["state"])
    if snap["history"] is not None:
        fresh.load_history(*snap["history"])
    fresh.load_series(*snap["series"])
    fresh.load_times(snap["times"] if snap["times"] is not None else np.zeros(0, np.int64))      # (a state without points exports no times)
    st.close()
    return fresh


def refused_call(engine, st, sc, op):
    variant = op["variant"]
    if variant == "dbscan_stream_without_history":
        stream_batch(engine, st, sc, op, "DBSCAN")
    elif variant == "num_keys_differs":
        stream_batch(engine, st, sc, op, "EWMA", num_keys=op["num_keys"])
    elif variant == "run_state_dbscan_without_history":
        engine.run_state(st, algo="DBSCAN")
    elif variant == "from_after_to":
        (engine.run_state_window if op["call"] == "window" else engine.drop_state)(st, *op["win"])
    elif variant == "start_time_in_run_state":
        engine._check(raw_run_state(engine, st, algo=0, start_time=op["start_time"]))
    else:
        raise ValueError(variant)


def execute(engine, st, sc, op):
    """one operation of a script on the state -> (the state, the call's own outputs in the form state_model.apply gives them)"""
    kind = op["kind"]
    if kind == "append":
        return st, {"rows": rows_of(stream_batch(engine, st, sc, op, op["algo"], **engine_params(op["algo"], op["params"])))}
    if kind in ("late", "refused"):
        try:
            if kind == "late":
                stream_batch(engine, st, sc, op, op["algo"], **engine_params(op["algo"], op["params"]))
            else:
                refused_call(engine, st, sc, op)
        except TadError:
            return st, {"raises": True}
        return st, {"raises": False}
    if kind == "merge":
        k, t, v = columns(engine, op)
        with engine.plan(**op["plan"]):
            return st, {"stats": engine.merge_stream(st, k, t, v, value_op=sc["op"], alpha=sc["alpha"], keep_from=op["keep_from"])}
    if kind == "trim":
        return st, {"dropped": st.trim(op["keep_points"], op["keep_from"], alpha=sc["alpha"])}
    if kind == "compact":
        remap, stats = st.compact(op["retire_before"])
        return st, {"remap": remap, "stats": stats}
    if kind == "resize":
        st.resize(op["n"])
        return st, {}
    if kind == "restart":
        return restart(engine, st, sc["flags"]), {}
    raise ValueError(kind)


def run_check(engine, st, check):
    p = engine_params(check["algo"], check["params"])
    call, win, emit_all = check["call"], check.get("win"), check["emit_all"]
    if call == "run_state":
        return engine.run_state(st, algo=check["algo"], emit_all=emit_all, **p)
    if call == "window":
        return engine.run_state_window(st, *win, algo=check["algo"], emit_all=emit_all, **p)
    if call == "keys":
        return engine.run_state_keys(st, check["mask"], *win, algo=check["algo"], emit_all=emit_all, **p)
    if call == "drop_state":
        return engine.drop_state(st, *win, emit_all=emit_all, **p)
    if call == "drop_state_keys":
        return engine.drop_state_keys(st, check["mask"], *win, emit_all=emit_all, **p)
    raise ValueError(call)


def replay(engine, seed, upto):
    """-> (state, model, script) as they are before operation `upto` of the seed's script; nothing is compared on the way"""
    sc = sm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for op in sc["ops"][:upto]:
        st, _ = execute(engine, st, sc, op)
        sm.apply(model, op, rows=False)
    return st, model, sc


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_sequence(engine, seed):
    sc = sm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], sm.describe(op))
        st, got = execute(engine, st, sc, op)
        want = sm.apply(model, op)
        # 1. the call's own outputs
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        if "raises" in want:
            assert got["raises"], (tag, "the call must be refused")
        if "rows" in want:
            assert_rows(got["rows"], want["rows"], (tag, "rows"))
        if op["kind"] == "merge":
            assert_counts(got["stats"], want["stats"], tag)
        if "dropped" in want:
            assert got["dropped"] == want["dropped"], (tag, got["dropped"], want["dropped"])
        if "remap" in want:
            assert np.array_equal(bits(got["remap"]), bits(want["remap"])), (tag, "remap")
            for f in COMPACT_FIELDS:
                assert got["stats"][f] == want["stats"][f], (tag, f, got["stats"][f], want["stats"][f])
        assert st.num_keys == model.num_keys, (tag, st.num_keys, model.num_keys)
        # 2. the whole state
        expected = model.expected_snapshot()
        assert_same(snapshot(st), expected, (tag, "state"))
        # 3. two read-only jobs
        for check in op["checks"]:
            ctag = (tag, check["call"], check["algo"], check["emit_all"], check["params"], check.get("win"), check.get("mask_kind"))
            res = run_check(engine, st, check)
            rows, counters = model.check_expect(check)
            assert_rows(rows_of(res), rows, ctag)
            for f, v in counters.items():
                assert res.stats[f] == v, (ctag, f, res.stats[f], v)
            assert res.stats["rows_in"] == res.stats["rows_used"] == counters["n_points"], ctag
        assert_same(snapshot(st), expected, (tag, "state after the read-only jobs"))
    st.close()
