#!/usr/bin/env python3
"""Timing of the streaming EWMA detector (tad_run_stream) on a day of second-resolution rows, device-resident columns.

Two shapes of a one-day table (default 1e8 rows, flowEndSeconds uniform over the day, gcd 1 s):
  pod   -- 1e5 keys, `sum` (the pod / svc shape);
  conn  -- 1e6 connection keys, `max` (the reference's default per-connection mode).
Each table is cut into 24 hourly and into 288 five-minute batches.  Every batch is timed three ways, alternating, in one process:
  (a) tad_run_stream as the engine plans it (sparse Stage 0 + k_stream_points where the sparse rule says so);
  (b) tad_run_stream forced dense (tad_plan.sparse = never) on a state of its own that advances in lockstep -- where the dense grid fits;
  (c) tad_run EWMA on the same batch (the batch job's per-batch cost).
Prints one JSON line: per shape and cut the medians over the batches (device time = tad_stats.ms_total, and wall time of the call) and
every batch's stage0_path and `identical` flag: (a)'s rows and state equal (b)'s bit for bit.
usage: python tools/stream_bench.py [--rows N] [--shapes pod,conn] [--cuts 3600,300]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine, TadError  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="pod,conn")
ap.add_argument("--cuts", default="3600,300", help="batch widths in seconds")
ap.add_argument("--seed", type=int, default=7)
args = ap.parse_args()

T0 = 1660202814
DAY = 86400
SHAPES = {"pod": (100_000, "svc", "sum"), "conn": (1_000_000, "", "max")}
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def windows(K, rows, seed, width=300):
    """the day as five-minute windows of host rows (rows within a window in arbitrary order)"""
    rng = np.random.default_rng(seed)
    nw = DAY // width
    per = np.full(nw, rows // nw, dtype=np.int64)
    per[: rows % nw] += 1
    out = []
    for w in range(nw):
        n = int(per[w])
        k = rng.integers(0, K, size=n, dtype=np.uint64)
        t = T0 + w * width + rng.integers(0, width, size=n).astype(np.int64)
        base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
        v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
        v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
        out.append((k, t, v))
    return out


def med(xs):
    xs = [x for x in xs if x is not None]
    return float(np.median(xs)) if xs else None


def same(a, b):
    return a.n_rows == b.n_rows and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def run_shape(eng, name, cut_widths):
    K, agg, op = SHAPES[name]
    wins = windows(K, args.rows, args.seed + K)
    out = {}
    for width in cut_widths:
        per_batch = width // 300
        batches = []
        for b in range(DAY // width):
            ws = wins[b * per_batch:(b + 1) * per_batch]
            batches.append(tuple(DeviceArray.from_host(eng, np.concatenate([w[i] for w in ws])) for i in range(3)))
        st_a, st_b = eng.state_create(K), eng.state_create(K)
        dense_ok = True
        rec = {"a_ms": [], "b_ms": [], "c_ms": [], "a_wall": [], "b_wall": [], "c_wall": [], "path": [], "identical": [], "rows": []}
        for dk, dt, dv in batches:
            t = time.perf_counter()
            a = eng.run_stream(st_a, dk, dt, dv, agg_flow=agg, value_op=op)
            rec["a_wall"].append((time.perf_counter() - t) * 1e3)
            rec["a_ms"].append(a.stats["ms_total"])
            rec["path"].append(a.stats["stage0_path"])
            rec["rows"].append(dk.n)
            b = None
            if dense_ok:
                try:
                    with eng.plan(sparse="never"):
                        t = time.perf_counter()
                        b = eng.run_stream(st_b, dk, dt, dv, agg_flow=agg, value_op=op)
                        rec["b_wall"].append((time.perf_counter() - t) * 1e3)
                    rec["b_ms"].append(b.stats["ms_total"])
                except TadError as exc:   # the dense grid does not fit: (b) is left out for this cut
                    dense_ok = False
                    rec["dense_error"] = exc.message[:160]
            if b is None:
                rec["b_ms"].append(None)
                rec["b_wall"].append(None)
            t = time.perf_counter()
            c = eng.run("EWMA", dk, dt, dv, K, agg_flow=agg, value_op=op)
            rec["c_wall"].append((time.perf_counter() - t) * 1e3)
            rec["c_ms"].append(c.stats["ms_total"])
            rec["identical"].append(None if b is None else bool(same(a, b)))
        if dense_ok:
            sa, sb = st_a.export(), st_b.export()
            rec["state_identical"] = all(np.array_equal(sa[f], sb[f]) for f in sa)
        st_a.close()
        st_b.close()
        for d in batches:
            for x in d:
                x.free()
        # the first batch of a cut carries the allocations: medians over the rest
        summary = {k: med(v[1:]) for k, v in rec.items() if k.endswith("_ms") or k.endswith("_wall")}
        summary.update({"batches": len(batches), "rows_per_batch": med(rec["rows"]), "paths": sorted(set(rec["path"])),
                        "all_identical": None if not dense_ok else all(rec["identical"]) and rec.get("state_identical", False),
                        "a_le_c": summary["a_ms"] <= summary["c_ms"],
                        "a_lt_b": None if summary["b_ms"] is None else summary["a_ms"] < summary["b_ms"]})
        summary["per_batch"] = {k: rec[k] for k in ("a_ms", "b_ms", "c_ms", "path", "identical")}
        if "dense_error" in rec:
            summary["dense_error"] = rec["dense_error"]
        out["%ds" % width] = summary
        print("# %s %ds: a %.3f ms  b %s ms  c %.3f ms  paths %s  identical %s" % (
            name, width, summary["a_ms"], "%.3f" % summary["b_ms"] if summary["b_ms"] is not None else "-", summary["c_ms"], summary["paths"],
            summary["all_identical"]), file=sys.stderr, flush=True)
    return out


def main():
    eng = TadEngine(device=0)
    cut_widths = [int(x) for x in args.cuts.split(",")]
    res = {"bench": "stream", "rows_per_day": args.rows, "shapes": {}}
    for name in args.shapes.split(","):
        K, agg, op = SHAPES[name]
        res["shapes"][name] = {"keys": K, "op": op, "cuts": run_shape(eng, name, cut_widths)}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
