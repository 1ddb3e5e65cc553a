#!/usr/bin/env python3
"""Timing of tad_run_state_buckets on a 24 h streaming state, device-resident columns.

The two 24 h states of tools/state_replace_bench.py (svc: 1e5 keys at minute resolution, sum; conn: 1e6 keys at second resolution, max),
judged in buckets of 60 s over the whole state and over the newest hour, EWMA and DBSCAN:
  (a) tad_run_state_buckets on the state;
  (b) tad_run over W'' — the window's points with their times floored, one row per point, held in device columns: Stage 0 plus the
      detectors on the same buckets;
  (c) once per case: the round trip there was before — export the state, floor the times in numpy, tad_run from host columns (wall clock).
Device time = the calls' ms_total (HIP events); median and range of --reps calls after an untimed pair whose rows are compared, (a) and (b)
alternating in ONE process.  --ab: instead, tad_run_state_window and tad_run_state_since alone (what a library of before this call has too),
for the parent A/B: run it once per library (TAD_LIBRARY_PATH), alternating processes, and compare the files.
Prints one JSON line and, with --out, writes it (profiles/state_buckets_bench.json).
usage: python tools/state_buckets_bench.py [--rows N] [--shapes svc,conn] [--reps R] [--ab] [--out PATH]"""
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
ALGOS = ("EWMA", "DBSCAN")
ROW_FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


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


def same_rows(a, b, what):
    for f in ROW_FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.size != y.size or not np.array_equal(x.view(np.uint64), y.view(np.uint64)):
            raise SystemExit("%s: the rows of the two paths differ in %s (%d vs %d rows)" % (what, f, x.size, y.size))


def build_state(eng, K, step, agg, op, seed):
    st = eng.state_create(K, history=True, series=True, times=True)
    for h in range(HOURS):
        rows = span_rows(K, step, args.rows, seed, T0 + h * HOUR, HOUR)
        d = tuple(DeviceArray.from_host(eng, x) for x in rows)
        eng.run_stream(st, *d, agg_flow=agg, value_op=op).close()
        for x in d:
            x.free()
    return st


def run_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    st = build_state(eng, K, step, agg, op, args.seed + K)
    end = T0 + HOURS * HOUR
    out = {"keys": K, "step_s": step, "op": op, "series_points": st.series_points(), "cases": {}}
    if args.ab:
        since = np.full(K, end - HOUR, np.int64)
        for algo in ALGOS:
            w, s = [], []
            for r in range(args.reps + 1):
                a = eng.run_state_window(st, from_t=end - 6 * HOUR, algo=algo, out="device")
                b = eng.run_state_since(st, key_since=since, from_t=end - 6 * HOUR, algo=algo, out="device")
                if r:
                    w.append(a.stats["ms_total"]), s.append(b.stats["ms_total"])
                a.close(), b.close()
            out["cases"][algo] = {"window_ms": summary(w), "since_ms": summary(s)}
        st.close()
        return out
    t = time.perf_counter()
    ln, vals = st.export_series()
    times = st.export_times()
    keys = np.repeat(np.arange(K, dtype=np.uint64), ln.astype(np.int64))
    export_ms = (time.perf_counter() - t) * 1e3
    for wname, from_t in (("whole", 0), ("newest_hour", end - HOUR)):
        t = time.perf_counter()
        sel = times >= from_t if from_t else np.ones(times.size, bool)
        wk, wt, wv = keys[sel], (times[sel] // args.bucket) * args.bucket, vals[sel]
        floor_ms = (time.perf_counter() - t) * 1e3
        d = tuple(DeviceArray.from_host(eng, np.ascontiguousarray(x)) for x in (wk, wt, wv))
        for algo in ALGOS:
            a_ms, b_ms = [], []
            for r in range(args.reps + 1):
                order = ("a", "b") if r % 2 == 0 else ("b", "a")
                res = {}
                for which in order:
                    if which == "a":
                        res["a"] = eng.run_state_buckets(st, args.bucket, 0, op, from_t=from_t, algo=algo, out="device")
                    else:
                        res["b"] = eng.run(algo, *d, K, agg_flow=agg, value_op=op, out="device")
                if r == 0:
                    same_rows(res["a"].to_host(), res["b"].to_host(), "%s %s %s" % (name, wname, algo))
                else:
                    a_ms.append(res["a"].stats["ms_total"]), b_ms.append(res["b"].stats["ms_total"])
                stats = {f: res["a"].stats[f] for f in ("rows_in", "n_points", "n_keys", "host_syncs")}
                rows = res["a"].n_rows
                res["a"].close(), res["b"].close()
            t = time.perf_counter()
            c = eng.run(algo, wk, wt, wv, K, agg_flow=agg, value_op=op, out="host")
            host_run_ms = (time.perf_counter() - t) * 1e3
            c.close()
            case = dict(stats, rows=int(rows), buckets_ms=summary(a_ms), tad_run_ms=summary(b_ms),
                        round_trip_ms={"export": export_ms, "floor": floor_ms, "tad_run_host_columns": host_run_ms})
            out["cases"]["%s/%s" % (wname, algo)] = case
            print("# %s %s %s: (a) %.3f ms [%.3f, %.3f], (b) %.3f ms [%.3f, %.3f], (c) %.0f ms; %d points -> %d buckets" %
                  (name, wname, algo, case["buckets_ms"]["median"], case["buckets_ms"]["min"], case["buckets_ms"]["max"], case["tad_run_ms"]["median"],
                   case["tad_run_ms"]["min"], case["tad_run_ms"]["max"], export_ms + floor_ms + host_run_ms, stats["rows_in"], stats["n_points"]),
                  file=sys.stderr, flush=True)
        if from_t:   # untimed, for a kernel trace: tad_run_state_window's gather of the same window beside the fold
            eng.run_state_window(st, from_t=from_t, algo="EWMA", out="device").close()
        for x in d:
            x.free()
    st.close()
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_buckets_parent_ab" if args.ab else "state_buckets", "rows_per_day": args.rows, "hours": HOURS, "reps": args.reps,
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
