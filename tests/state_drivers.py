"""What drives a TadState next to its host model, shared by the sequence, replace, change-report and rollup tests: one operation of a
script executed on both sides and compared (`execute`, `run_check`, `restart`), the rollup pair (`build`, `roll`), and the builders of
the replace tests.  state_helpers.py holds what needs no model."""
import numpy as np

import replace_model as rm
import rollup_model as R
from rollup_model import RollupModel
from state_helpers import HIST, I64, SER, TIMES, U64, assert_same, new_state, raw_run_state, rows_of, snapshot, window
from theia_amd import TadError
from theia_amd.engine import DeviceArray

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


def reloaded(engine, st, flags):
    """a fresh state that imported every part st exports"""
    snap = snapshot(st)
    fresh = new_state(engine, st.num_keys, flags)
    fresh.load(snap["state"])
    if snap["history"] is not None:
        fresh.load_history(*snap["history"])
    fresh.load_series(*snap["series"])
    fresh.load_times(snap["times"] if snap["times"] is not None else np.zeros(0, I64))      # (a state without points exports no times)
    return fresh


def restart(engine, st, flags):
    """export every part, a fresh state, import: the host restarted"""
    fresh = reloaded(engine, st, flags)
    st.close()
    return fresh


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


def assert_stats(got, want, what):
    for f in R.STATS:
        assert got[f] == want[f], (what, f, got[f], want[f], got, want)


def build(engine, K, k, t, v, op="sum", alpha=0.0, history=True, seed=1):
    """a state of K keys fed the points (k, t, v), one row each, in a seeded order -> (state, its model)"""
    k, t, v = np.asarray(k).astype(U64), np.asarray(t, I64), np.asarray(v).astype(U64)
    flags = SER | TIMES | (HIST if history else 0)
    st = new_state(engine, K, flags)
    if k.size:
        o = np.random.default_rng(seed).permutation(k.size)
        engine.run_stream(st, np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o]), value_op=op, alpha=alpha)
    m = RollupModel(K, flags, op, alpha)
    if k.size:
        m._set(*window(st))
    assert_same(snapshot(st), m.expected_snapshot(), "the state as built")
    return st, m


def roll(st, m, before, bucket_s, origin=0, op=None, what="", alpha=None, expected=None):
    """the call on state and model, everything compared; then the same call again, which must change no bit -> the first call's stats"""
    op = op or m.op
    alpha = m.alpha if alpha is None else alpha
    want = m.rollup(before, bucket_s, origin, op)
    got = st.rollup(before, bucket_s, origin, op, alpha)
    assert_stats(got, want, what)
    assert got["points_after"] == st.series_points() == m.key.size, what
    exp = expected() if expected else m.expected_snapshot()
    snap = snapshot(st)
    assert_same(snap, exp, (what, "state"))
    again = st.rollup(before, bucket_s, origin, op, alpha)
    assert_same(snapshot(st), snap, (what, "the second call changed a bit"))
    assert again["keys_changed"] == 0 and again["points_before"] == again["points_after"] == got["points_after"], (what, again)
    assert again["points_rolled"] == again["buckets"] == got["buckets"] and again["before_t"] == got["before_t"], (what, again)
    return got


T0 = 1_700_000_000
FIVE = np.array([(1 << 61) + 12345, (1 << 55) + 7, (1 << 58) + 999, (1 << 50) + 1, (1 << 60) + 31], U64)


def old_values(rng, n, flags):
    return FIVE[rng.integers(0, 5, size=n)] if flags & HIST else big(rng, n)


def big(rng, n):
    """n values of 50 to 62 significant bits"""
    b = rng.integers(49, 62, size=n).astype(U64)
    return (U64(1) << b) | (rng.integers(0, 1 << 62, size=n, dtype=U64) & ((U64(1) << b) - U64(1)))


def table_of(lens, rng, flags):
    """point i of key j at T0 + 2 i"""
    lens = np.asarray(lens, I64)
    k = np.repeat(np.arange(lens.size, dtype=U64), lens)
    i = np.concatenate([np.arange(n, dtype=I64) for n in lens]) if lens.sum() else np.zeros(0, I64)
    return k, T0 + 2 * i, old_values(rng, k.size, flags)


def clone(engine, st, model, flags):
    """a fresh state and a fresh model holding what (st, model) hold: the edge loops start every case from the same table"""
    m = rm.ReplaceModel(model.num_keys, model.flags, model.op, model.alpha)
    m._set(*model.points())
    return reloaded(engine, st, flags), m


def execute_any(engine, st, sc, op):
    if op["kind"] != "replace":
        return execute(engine, st, sc, op)
    cols = op["cols"]
    k, t, v = op["k"], op["t"], op["v"]
    if cols == "host4":
        k, t = k.astype(np.uint32), t.astype(np.uint32)
    elif cols == "device":
        k, t, v = (DeviceArray.from_host(engine, a) for a in (k, t, v))
    with engine.plan(**op["plan"]):
        return st, {"stats": engine.replace_stream(st, k, t, v, from_t=op["from_t"], to_t=op["to_t"], ranged=op["ranged"], value_op=sc["op"],
                                                   alpha=sc["alpha"], keep_from=op["keep_from"])}
