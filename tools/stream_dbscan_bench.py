#!/usr/bin/env python3
"""Timing of the streaming DBSCAN detector (tad_run_stream with TAD_ALGO_DBSCAN on a state with history), device-resident columns.

Two shapes of a one-day table (default 1e8 rows) in 24 hourly batches:
  svc   -- 1e5 keys at minute resolution, `sum` (the svc / pod shape);
  conn  -- 1e6 connection keys at second resolution, `max`.
Per batch: the tad_run_stream DBSCAN time (device = tad_stats.ms_total, and wall), the history's points and bytes (two copies of 8 B a
point: a batch merges into the second one).  At batches 1, 6, 12 and 24 also tad_run DBSCAN over the accumulated window -- what a caller
pays today for the same verdicts -- and whether its rows for the batch's points equal the stream's bit for bit.
--save-before-last PATH: stop before the last batch and save the state (moments + history) and nothing else is timed;
--resume PATH: load that state into a fresh history state and run the last batch alone (for `rocprofv3 --kernel-trace --stats`).
Prints one JSON line.
usage: python tools/stream_dbscan_bench.py [--rows N] [--shapes svc,conn] [--save-before-last P | --resume P]"""
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
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--save-before-last", default=None)
ap.add_argument("--resume", default=None)
args = ap.parse_args()

T0 = 1660202814
DAY, HOUR = 86400, 3600
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
CHECK = (1, 6, 12, 24)
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def hour(K, step, rows, seed, h):
    """the rows of hour h (host), in arbitrary order: every key's values around a base of its own, one in 1e3 a spike"""
    rng = np.random.default_rng(seed * 1000 + h)
    n = rows // 24 + (1 if h < rows % 24 else 0)
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    t = T0 + h * HOUR + step * rng.integers(0, HOUR // step, size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def codes(k, t):
    return (np.asarray(k, np.uint64) << np.uint64(32)) | (np.asarray(t, np.int64) - T0).astype(np.uint64)


def run_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    hours = [hour(K, step, args.rows, args.seed + K, h) for h in range(24)]
    st = eng.state_create(K, history=True)
    first = 0
    if args.resume:
        z = np.load(args.resume)
        st.load({f: z[f] for f in ("n", "avg", "m2", "ewma", "last_t")})
        st.load_history(z["len"], z["values"])
        first = 23
    rec = {"stream_ms": [], "stream_wall_ms": [], "rows_out": [], "history_points": [], "history_bytes": [], "stage0_path": [], "batch_job": {}}
    for h in range(first, 24):
        if args.save_before_last and h == 23:
            s = st.export()
            ln, vals = st.export_history()
            np.savez(args.save_before_last, len=ln, values=vals, **s)
            break
        d = tuple(DeviceArray.from_host(eng, x) for x in hours[h])
        t = time.perf_counter()
        r = eng.run_stream(st, *d, agg_flow=agg, value_op=op, algo="DBSCAN")
        rec["stream_wall_ms"].append((time.perf_counter() - t) * 1e3)
        rec["stream_ms"].append(r.stats["ms_total"])
        rec["stage0_path"].append(r.stats["stage0_path"])
        rec["rows_out"].append(r.n_rows)
        hp = st.history_points()
        rec["history_points"].append(hp)
        rec["history_bytes"].append(hp * 16)
        got = r.to_host()
        for x in d:
            x.free()
        if h + 1 in CHECK and not args.resume and not args.save_before_last:
            acc = tuple(DeviceArray.from_host(eng, np.concatenate([hh[i] for hh in hours[:h + 1]])) for i in range(3))
            eng.run("DBSCAN", *acc, K, agg_flow=agg, value_op=op).close()   # (warm: the workspace of this window's size)
            t = time.perf_counter()
            b = eng.run("DBSCAN", *acc, K, agg_flow=agg, value_op=op)
            wall = (time.perf_counter() - t) * 1e3
            bh = b.to_host()
            sel = np.isin(codes(bh["key_id"], bh["flow_end_s"]), np.unique(codes(hours[h][0], hours[h][1])))
            same = int(sel.sum()) == r.n_rows and all(np.array_equal(bh[f][sel].view(np.uint64), got[f].view(np.uint64)) for f in FIELDS)
            rec["batch_job"][str(h + 1)] = {"ms": b.stats["ms_total"], "wall_ms": wall, "rows_in": int(acc[0].n), "stage0_path": b.stats["stage0_path"],
                                            "identical": bool(same), "stream_ms": rec["stream_ms"][-1]}
            print("# %s batch %d: stream %.3f ms, tad_run over %d rows %.3f ms, identical %s" % (
                name, h + 1, rec["stream_ms"][-1], acc[0].n, b.stats["ms_total"], same), file=sys.stderr, flush=True)
            for x in acc:
                x.free()
    st.close()
    return {"keys": K, "step_s": step, "op": op, **rec}


def main():
    eng = TadEngine(device=0)
    res = {"bench": "stream_dbscan", "rows_per_day": args.rows, "batches": 24, "resume": bool(args.resume), "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_shape(eng, name)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
