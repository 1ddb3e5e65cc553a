#!/usr/bin/env python3
"""Timing of tad_state_merge against what a caller can do without it, device-resident columns.

The two shapes of tools/stream_trim_bench.py (1e8 rows a day in hourly batches):
  svc   -- 1e5 keys at minute resolution, `sum`;
  conn  -- 1e6 connection keys at second resolution, `max`;
on a TAD_STATE_HISTORY | SERIES | TIMES state (flags 11) and on a SERIES | TIMES state (flags 10).  Hours 0-23 are streamed in with
tad_run_stream; the state is exported once (the snapshot every timed call starts from); then the next batch in three forms:
  i    -- hour 24, in order;
  ii   -- hour 24 with 2 % of its rows replaced by new rows at times of hours 21-23 (late);
  iii  -- hour 23 sent again (every point combines).
Timed, alternating in one process, --reps times each, every call from the restored snapshot:
  a -- tad_state_merge of the batch;
  b -- the twin: tad_run_stream EWMA of the batch (form i only: it refuses the others);
  c -- what a caller has to do today for ii / iii: a fresh state and ONE tad_run_stream batch over W ++ B, W = the raw rows of hours 0-23
       already in device columns (generous to c, which in reality also has to fetch those rows again).
Before anything is timed the state (a) leaves is compared bit for bit with (b)'s for form i and with (c)'s — which is R1 of the call's
contract — for forms ii and iii.  Prints one JSON line: medians and min-max of ms_total (HIP events) per shape, flags, form and method.
--profile FORM: stream the 24 hours in, run exactly ONE merge of that form and exit (for `rocprofv3 --kernel-trace --stats --`: the
k_merge_* and k_hist_subtract rows of the statistics are then that call's).
usage: python tools/stream_merge_bench.py [--rows N] [--shapes svc,conn] [--flags 11,10] [--reps R] [--profile i|ii|iii]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn")
ap.add_argument("--flags", default="11,10")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--profile", default="")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
HOURS = 24
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
STATE_FIELDS = ("n", "avg", "m2", "ewma", "last_t")


def hour(K, step, rows, seed, h, t_lo=None, n=None):
    """the rows of hour h (host), in arbitrary order, as tools/stream_trim_bench.py makes them; t_lo: the times from that hour on instead"""
    rng = np.random.default_rng(seed * 1000 + h)
    if n is None:
        n = rows // 24 + (1 if h % 24 < rows % 24 else 0)
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    span = HOUR if t_lo is None else 3 * HOUR
    t = T0 + (h if t_lo is None else t_lo) * HOUR + step * rng.integers(0, span // step, size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def snapshot(st):
    return {"state": st.export(), "series": st.export_series(), "times": st.export_times(), "history": st.export_history() if st.history else None}


def restore(eng, K, flags, snap):
    st = eng.state_create(K, history=bool(flags & 1), series=True, times=True)
    st.load(snap["state"])
    st.load_series(*snap["series"])
    st.load_times(snap["times"])
    if snap["history"] is not None:
        st.load_history(*snap["history"])
    return st


def same(a, b):
    ok = all(np.array_equal(a["state"][f].view(np.uint64) if a["state"][f].dtype.itemsize == 8 else a["state"][f],
                            b["state"][f].view(np.uint64) if b["state"][f].dtype.itemsize == 8 else b["state"][f]) for f in STATE_FIELDS)
    ok = ok and np.array_equal(a["series"][0], b["series"][0]) and np.array_equal(a["series"][1], b["series"][1]) and np.array_equal(a["times"], b["times"])
    if a["history"] is not None:
        ok = ok and np.array_equal(a["history"][0], b["history"][0]) and np.array_equal(a["history"][1], b["history"][1])
    return bool(ok)


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def run_shape(eng, name, flags):
    K, step, agg, op = SHAPES[name]
    seed = args.seed + K
    hrs = [hour(K, step, args.rows, seed, h) for h in range(HOURS + 1)]
    st = eng.state_create(K, history=bool(flags & 1), series=True, times=True)
    for h in range(HOURS):
        d = tuple(DeviceArray.from_host(eng, x) for x in hrs[h])
        eng.run_stream(st, *d, agg_flow=agg, value_op=op).close()
        for x in d:
            x.free()
    n24 = hrs[HOURS][0].size
    n_late = n24 // 50
    late = hour(K, step, args.rows, seed, 1000, t_lo=HOURS - 3, n=n_late)
    forms = {"i": hrs[HOURS], "ii": tuple(np.concatenate([hrs[HOURS][i][n_late:], late[i]]) for i in range(3)), "iii": hrs[HOURS - 1]}
    if args.profile:
        d = tuple(DeviceArray.from_host(eng, x) for x in forms[args.profile])
        s = eng.merge_stream(st, *d, agg_flow=agg, value_op=op)
        print("# profile %s flags %d form %s: %s" % (name, flags, args.profile, s), file=sys.stderr, flush=True)
        st.close()
        return {"keys": K, "profile": args.profile, "stats": s}
    snap = snapshot(st)
    st.close()
    dev = {f: tuple(DeviceArray.from_host(eng, x) for x in rows) for f, rows in forms.items()}
    W = tuple(np.concatenate([hrs[h][i] for h in range(HOURS)]) for i in range(3))
    dev_wb = {f: tuple(DeviceArray.from_host(eng, np.concatenate([W[i], forms[f][i]])) for i in range(3)) for f in ("ii", "iii")}
    del W, hrs

    def method_a(f):
        s = restore(eng, K, flags, snap)
        stats = eng.merge_stream(s, *dev[f], agg_flow=agg, value_op=op)
        return s, stats

    def method_b(f):
        s = restore(eng, K, flags, snap)
        r = eng.run_stream(s, *dev[f], agg_flow=agg, value_op=op)
        ms = r.stats["ms_total"]
        r.close()
        return s, ms

    def method_c(f):
        s = eng.state_create(K, history=bool(flags & 1), series=True, times=True)
        r = eng.run_stream(s, *dev_wb[f], agg_flow=agg, value_op=op)
        ms = r.stats["ms_total"]
        r.close()
        return s, ms

    out = {"keys": K, "step_s": step, "op": op, "flags": flags, "window_points": int(snap["times"].size), "forms": {}}
    # the bit-identity check, before anything is timed
    for f in ("i", "ii", "iii"):
        sa, stats = method_a(f)
        sb, _ = method_b(f) if f == "i" else method_c(f)
        ident = same(snapshot(sa), snapshot(sb))
        sa.close()
        sb.close()
        out["forms"][f] = {"identical": ident, "rows": int(dev[f][0].n),
                           "stats": {k: v for k, v in stats.items() if not k.startswith("ms_")}, "a": [], "b": [], "c": [], "a_stage0": [], "a_merge": []}
        print("# %s flags %d form %s: identical %s, %s" % (name, flags, f, ident, out["forms"][f]["stats"]), file=sys.stderr, flush=True)
    for _ in range(args.reps):
        for f in ("i", "ii", "iii"):
            rec = out["forms"][f]
            sa, stats = method_a(f)
            sa.close()
            rec["a"].append(stats["ms_total"])
            rec["a_stage0"].append(stats["ms_stage0"])
            rec["a_merge"].append(stats["ms_merge"])
            sb, ms = method_b(f) if f == "i" else method_c(f)
            sb.close()
            rec["b" if f == "i" else "c"].append(ms)
    for f, rec in out["forms"].items():
        for m in ("a", "b", "c", "a_stage0", "a_merge"):
            rec[m] = summary(rec[m]) if rec[m] else None
        print("# %s flags %d form %s: a %s, b %s, c %s" % (name, flags, f, rec["a"], rec["b"], rec["c"]), file=sys.stderr, flush=True)
    for cols in list(dev.values()) + list(dev_wb.values()):
        for x in cols:
            x.free()
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "stream_merge", "rows_per_day": args.rows, "reps": args.reps, "results": []}
    for name in args.shapes.split(","):
        for flags in (int(x) for x in args.flags.split(",")):
            r = run_shape(eng, name, flags)
            r["shape"] = name
            res["results"].append(r)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
