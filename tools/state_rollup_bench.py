#!/usr/bin/env python3
"""Timing of tad_state_rollup on a 24 h streaming state.

The two 24 h states of tools/state_replace_bench.py (svc: 1e5 keys at minute resolution, sum; conn: 1e6 keys at second resolution, max).
Two roll-ups each, at --bucket seconds:
  first   "everything older than the newest hour" on the raw state;
  steady  the steady state of a periodic roll-up: everything older than the newest TWO hours is rolled already, one more hour is rolled.
Against:
  (a) tad_state_trim at the same bound on the same state: the cheapest rewrite of the same arenas, so the roll-up's price for keeping the
      data is the difference;
  (b) once per case: the route there was before — export the state, floor and fold in numpy, import (wall clock).
A roll-up and a trim change the state, so every repetition starts from the case's snapshot, imported anew (untimed).  Device time = the
roll-up's ms_total (HIP events); the trim reports no device time, so both calls' wall clock is taken too (each ends with its own
stream synchronisation) and the trim is compared on that; median and range of --reps calls after an
untimed one whose export is compared with (b)'s.  tad_state_bytes before and after.  --ab: instead, tad_run_state_buckets (EWMA, whole
state) alone — what a library of before this call has too — for the parent A/B: run it once per library (TAD_LIBRARY_PATH), alternating
processes, and compare the files.
Prints one JSON line and, with --out, writes it (profiles/state_rollup_bench.json).
usage: python tools/state_rollup_bench.py [--rows N] [--shapes svc,conn] [--reps R] [--bucket S] [--ab] [--out PATH]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--bucket", type=int, default=60)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()

T0 = 1660202814
HOUR, MINUTE, HOURS = 3600, 60, 24
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op


def span_rows(K, step, rows_per_day, seed, t_from, seconds):
    """the table's rows with flowEndSeconds in [t_from, t_from + seconds) (tools/state_replace_bench.py's generator)"""
    rng = np.random.default_rng(seed * 100_000 + (t_from - T0) // MINUTE)
    n = max(1, rows_per_day * seconds // (HOURS * HOUR))
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    t = t_from + step * rng.integers(0, max(1, seconds // step), size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def build_state(eng, K, step, agg, op, seed):
    st = eng.state_create(K, history=True, series=True, times=True)
    for h in range(HOURS):
        rows = span_rows(K, step, args.rows, seed, T0 + h * HOUR, HOUR)
        d = tuple(DeviceArray.from_host(eng, x) for x in rows)
        eng.run_stream(st, *d, agg_flow=agg, value_op=op).close()
        for x in d:
            x.free()
    return st


def export(st):
    return {"state": st.export(), "history": st.export_history(), "series": st.export_series(), "times": st.export_times()}


def restore(eng, K, snap):
    st = eng.state_create(K, history=True, series=True, times=True)
    st.load(snap["state"]), st.load_history(*snap["history"]), st.load_series(*snap["series"]), st.load_times(snap["times"])
    return st


def same(a, b, what):
    for f in ("n", "avg", "m2", "last_t"):      # (ewma of a key that lost no point is the stored one: not the host route's replay)
        if not np.array_equal(np.ascontiguousarray(a["state"][f]).view(np.uint8), np.ascontiguousarray(b["state"][f]).view(np.uint8)):
            raise SystemExit("%s: the two routes differ in %s" % (what, f))
    for part in ("history", "series"):
        if not (np.array_equal(a[part][0], b[part][0]) and np.array_equal(a[part][1], b[part][1])):
            raise SystemExit("%s: the two routes differ in the %s" % (what, part))
    if not np.array_equal(a["times"], b["times"]):
        raise SystemExit("%s: the two routes differ in the times" % what)


def host_route(eng, K, snap, bound, op):
    """(b): export is `snap` already (its time is measured by the caller); floor and fold in numpy, a fresh state, one stream batch"""
    t = time.perf_counter()
    ln, vals = snap["series"]
    times = snap["times"]
    keys = np.repeat(np.arange(K, dtype=np.uint64), ln.astype(np.int64))
    t2 = np.where(times < bound, (times // args.bucket) * args.bucket, times)
    head = np.ones(keys.size, bool)
    head[1:] = (keys[1:] != keys[:-1]) | (t2[1:] != t2[:-1])
    first = np.flatnonzero(head)
    with np.errstate(over="ignore"):
        v2 = np.add.reduceat(vals, first) if op == "sum" else np.maximum.reduceat(vals, first)
    fold_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    st = eng.state_create(K, history=True, series=True, times=True)
    eng.run_stream(st, keys[first], t2[first], v2.astype(np.uint64), value_op=op).close()
    import_ms = (time.perf_counter() - t) * 1e3
    return st, fold_ms, import_ms


def wall_ms(fn):
    """fn() -> (its wall clock in ms, its result): both calls end with their own stream synchronisation"""
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def run_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    st = build_state(eng, K, step, agg, op, args.seed + K)
    end = T0 + HOURS * HOUR
    out = {"keys": K, "step_s": step, "op": op, "series_points": st.series_points(), "cases": {}}
    if args.ab:
        ms = []
        for r in range(args.reps + 1):
            a = eng.run_state_buckets(st, args.bucket, 0, op, algo="EWMA", out="device")
            if r:
                ms.append(a.stats["ms_total"])
            a.close()
        out["cases"]["buckets_whole_EWMA_ms"] = summary(ms)
        st.close()
        return out
    t = time.perf_counter()
    raw = export(st)
    export_ms = (time.perf_counter() - t) * 1e3
    st.rollup(end - 2 * HOUR, args.bucket, 0, op)
    rolled = export(st)
    st.close()
    for cname, snap in (("first", raw), ("steady", rolled)):
        bound = end - HOUR
        ref, fold_ms, import_ms = host_route(eng, K, snap, bound // args.bucket * args.bucket, op)
        want = export(ref)
        ref.close()
        roll_ms, roll_wall, trim_ms, case = [], [], [], {}
        for r in range(args.reps + 1):
            s = restore(eng, K, snap)
            before = s.nbytes()
            wall, rs = wall_ms(lambda: s.rollup(bound, args.bucket, 0, op))
            if r == 0:
                same(export(s), want, "%s %s" % (name, cname))
                case = {f: rs[f] for f in ("points_before", "points_after", "points_rolled", "buckets", "keys_changed", "before_t")}
                case.update(bytes_before=before, bytes_after=s.nbytes())
            else:
                roll_ms.append(rs["ms_total"]), roll_wall.append(wall)
            s.close()
            s = restore(eng, K, snap)
            ms, dropped = wall_ms(lambda: s.trim(0, rs["before_t"]))
            if r:
                trim_ms.append(ms)
            else:
                case.update(trim_dropped=dropped, trim_bytes_after=s.nbytes())
            s.close()
        case.update(rollup_ms=summary(roll_ms), rollup_wall_ms=summary(roll_wall), trim_wall_ms=summary(trim_ms), host_route_ms={"export": export_ms, "fold": fold_ms, "import": import_ms})
        out["cases"][cname] = case
        print("# %s %s: roll-up %.3f ms [%.3f, %.3f] (wall %.3f), trim wall %.3f ms [%.3f, %.3f], host route %.0f ms; %d -> %d points, %d -> %d bytes" %
              (name, cname, case["rollup_ms"]["median"], case["rollup_ms"]["min"], case["rollup_ms"]["max"], case["rollup_wall_ms"]["median"],
               case["trim_wall_ms"]["median"], case["trim_wall_ms"]["min"], case["trim_wall_ms"]["max"], export_ms + fold_ms + import_ms, case["points_before"], case["points_after"],
               case["bytes_before"], case["bytes_after"]), file=sys.stderr, flush=True)
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_rollup_parent_ab" if args.ab else "state_rollup", "rows_per_day": args.rows, "hours": HOURS, "reps": args.reps,
           "bucket_s": args.bucket, "library": os.path.basename(os.environ.get("TAD_LIBRARY_PATH", "")), "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_shape(eng, name)
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
