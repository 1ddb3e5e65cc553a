#!/usr/bin/env python3
"""Timing of the alert turn of a poll loop on a 24 h streaming state, device-resident columns.

The two 24 h states of tools/state_replace_bench.py (svc: 1e5 keys at minute resolution, sum; conn: 1e6 keys at second resolution, max).
One TURN re-reads the last 5 minutes, of which the newest minute is new rows: turn r replaces [end + (r - 4) min, end + (r + 1) min) with
every row of those seconds.  Two twin states take the same turns, alternating per turn, in ONE process:
  (a) tad_state_replace_changes (report on the device) + tad_run_state_since with the report's key_since — EWMA and DBSCAN on both
      states, ARIMA on the svc state over each key's newest 100 points;
  (b) what there was before: tad_state_replace + tad_run_state_window over everything (ARIMA: keep_points = 100) + a host filter of
      the rows (flow_end_s >= the re-read's from_t);
  (c) falls out of the two: tad_state_replace alone (b) against tad_state_replace_changes (a) on the same batch.
Device time = the calls' ms_total (HIP events); medians and ranges over --reps turns after an untimed first turn whose rows are compared:
(a)'s rows must be (b)'s rows restricted to the report's keys and times.  Prints one JSON line and, with --out, writes it
(profiles/state_alerts_bench.json).
usage: python tools/state_alerts_bench.py [--rows N] [--shapes svc,conn] [--reps R] [--out PATH]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine, _capi  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", default="")
args = ap.parse_args()

T0 = 1660202814
HOUR, MINUTE, HOURS = 3600, 60, 24
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
ALGOS = {"svc": ("EWMA", "DBSCAN", "ARIMA"), "conn": ("EWMA", "DBSCAN")}
ROW_FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def span_rows(K, step, rows_per_day, seed, t_from, seconds):
    """the table's rows with flowEndSeconds in [t_from, t_from + seconds): a function of (seed, t_from), in arbitrary order"""
    rng = np.random.default_rng(seed * 100_000 + (t_from - T0) // MINUTE)
    n = max(1, rows_per_day * seconds // (HOURS * HOUR))
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    t = t_from + step * rng.integers(0, max(1, seconds // step), size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def minutes(K, step, seed, first, count):
    parts = [span_rows(K, step, args.rows, seed, first + i * MINUTE, MINUTE) for i in range(count)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def run_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    seed = args.seed + K
    sa = eng.state_create(K, history=True, series=True, times=True)
    sb = eng.state_create(K, history=True, series=True, times=True)
    for h in range(HOURS):
        rows = minutes(K, step, seed, T0 + h * HOUR, 60)
        d = tuple(DeviceArray.from_host(eng, x) for x in rows)
        for s in (sa, sb):
            eng.run_stream(s, *d, agg_flow=agg, value_op=op).close()
        for x in d:
            x.free()
    end = T0 + HOURS * HOUR
    out = {"keys": K, "step_s": step, "op": op, "series_points": sa.series_points(), "algos": {}}
    rec = {"replace_changes_ms": [], "replace_ms": []}
    for algo in ALGOS[name]:
        rec[algo] = {"since_ms": [], "window_ms": [], "filter_ms": [], "rows_since": [], "rows_window": []}
    for r in range(args.reps + 1):
        from_t, to_t = end + (r - 4) * MINUTE, end + (r + 1) * MINUTE
        batch = minutes(K, step, seed, from_t, 5)
        d = tuple(DeviceArray.from_host(eng, x) for x in batch)
        order = ("a", "b") if r % 2 == 0 else ("b", "a")
        for which in order:
            if which == "a":
                st = eng.replace_stream_changes(sa, *d, "device", from_t=from_t, to_t=to_t, ranged=True, agg_flow=agg, value_op=op)
                since = st["key_since"]
                res_a = {}
                for algo in ALGOS[name]:
                    kp = 100 if algo == "ARIMA" else 0
                    res = eng.run_state_since(sa, key_since=since, keep_points=kp, algo=algo, out="device")
                    res_a[algo] = res
                    if r:
                        rec[algo]["since_ms"].append(res.stats["ms_total"])
                        rec[algo]["rows_since"].append(res.n_rows)
                if r:
                    rec["replace_changes_ms"].append(st["ms_total"])
                changes = {f: st[f] for f in ("keys_changed", "points_changed", "keys_touched", "points_replaced", "points_appended")}
            else:
                st = eng.replace_stream(sb, *d, from_t=from_t, to_t=to_t, ranged=True, agg_flow=agg, value_op=op)
                res_b = {}
                for algo in ALGOS[name]:
                    kp = 100 if algo == "ARIMA" else 0
                    res = eng.run_state_window(sb, keep_points=kp, algo=algo, out="host")
                    t = time.perf_counter()
                    sel = np.asarray(res["flow_end_s"]) >= from_t
                    kept = {f: np.asarray(res[f])[sel] for f in ROW_FIELDS}
                    fms = (time.perf_counter() - t) * 1e3
                    res_b[algo] = (res, kept)
                    if r:
                        rec[algo]["window_ms"].append(res.stats["ms_total"])
                        rec[algo]["filter_ms"].append(fms)
                        rec[algo]["rows_window"].append(res.n_rows)
                if r:
                    rec["replace_ms"].append(st["ms_total"])
        if r == 0:   # the untimed pair: (a)'s rows are (b)'s rows of the changed keys from their changed time on
            ks = since.to_host()
            for algo in ALGOS[name]:
                full = res_b[algo][0]
                k = np.asarray(full["key_id"]).astype(np.int64)
                sel = (ks[k] != _capi.TAD_NO_CHANGE) & (np.asarray(full["flow_end_s"]) >= ks[k])
                got = res_a[algo].to_host()
                for f in ROW_FIELDS:
                    a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(np.asarray(full[f])[sel])
                    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                        raise SystemExit("%s %s: the rows of the two paths differ in %s (%d vs %d rows)" % (name, algo, f, a.size, b.size))
            out["first_turn"] = dict(changes, rows={algo: int(res_a[algo].n_rows) for algo in ALGOS[name]})
        out["last_turn"] = changes
        since.free()
        for res in res_a.values():
            res.close()
        for res, _ in res_b.values():
            res.close()
        for x in d:
            x.free()
    out["replace_changes_ms"], out["replace_ms"] = summary(rec["replace_changes_ms"]), summary(rec["replace_ms"])
    for algo in ALGOS[name]:
        a = rec[algo]
        out["algos"][algo] = {"since_ms": summary(a["since_ms"]), "window_ms": summary(a["window_ms"]), "host_filter_ms": summary(a["filter_ms"]),
                              "rows_since_median": float(np.median(a["rows_since"])), "rows_window_median": float(np.median(a["rows_window"])),
                              "turn_a_ms_median": out["replace_changes_ms"]["median"] + float(np.median(a["since_ms"])),
                              "turn_b_ms_median": out["replace_ms"]["median"] + float(np.median(a["window_ms"])) + float(np.median(a["filter_ms"]))}
        print("# %s %s: (a) %.3f + %.3f ms, (b) %.3f + %.3f + %.3f ms" % (name, algo, out["replace_changes_ms"]["median"], np.median(a["since_ms"]),
              out["replace_ms"]["median"], np.median(a["window_ms"]), np.median(a["filter_ms"])), file=sys.stderr, flush=True)
    sa.close()
    sb.close()
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_alerts", "rows_per_day": args.rows, "hours": HOURS, "reps": args.reps, "shapes": {}}
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
