#!/usr/bin/env python3
"""Timing of a re-read that replaces (tad_state_replace) on a 24 h streaming state, device-resident columns.

The two 24 h shapes of tools/stream_trim_bench.py (1e8 rows a day, fed in hourly batches):
  svc   -- 1e5 keys at minute resolution, `sum`;
  conn  -- 1e6 connection keys at second resolution, `max`.
The batch is a re-read of the day's last 5 minutes and of its last hour: every row of the table with flowEndSeconds in the range, so every
point of the batch replaces a point the state holds and nothing is erased — the poll loop's common turn.  Timed in ONE process, alternating
per repetition, on states that hold the same day:
  (a) tad_state_replace, ranged over the re-read seconds, on a state with history, series and times;
  (b) tad_state_merge of the same batch on a twin state with `max` — the same placement work through the existing call (idempotent under
      max, so the twin holds the same points at every repetition);
  (c) the same change made on the host: export (moments, series, times, history) -> numpy (drop the range, place the batch's aggregated
      points, re-sort the history per key) -> import.  A LOWER bound of what a host would pay: the replay of the touched keys' moments
      (avg, m2, ewma) is left out, only n is brought up to date, because the import checks it.
Medians over --reps repetitions with the first call of each left out ((c): --host-reps); device time = the call's ms_total, wall = around
the call.  Prints one JSON line and, with --out, writes it (profiles/state_replace_bench.json).
usage: python tools/state_replace_bench.py [--rows N] [--shapes svc,conn] [--reps R] [--host-reps H] [--out PATH]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", default="")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
HOURS = 24
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
REREADS = {"5min": 300, "1h": 3600}


def hour(K, step, rows, seed, h):
    """tools/stream_trim_bench.py's rows of hour h (host), in arbitrary order"""
    rng = np.random.default_rng(seed * 1000 + h)
    n = rows // 24 + (1 if h % 24 < rows % 24 else 0)
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    t = T0 + h * HOUR + step * rng.integers(0, HOUR // step, size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def median_after_first(xs):
    return float(np.median(xs[1:])) if len(xs) > 1 else float(xs[0])


def host_change(st, batch, from_t, to_t, op):
    """(c): the replace made on the host.  -> seconds per phase"""
    t0 = time.perf_counter()
    mom = st.export()
    ln, vals = st.export_series()
    times = st.export_times()
    st.export_history()
    t1 = time.perf_counter()
    K = ln.size
    keys = np.repeat(np.arange(K, dtype=np.uint64), ln.astype(np.int64))
    keep = ~((times >= from_t) & (times < to_t))
    bk, bt, bv = batch
    code = (bk << np.uint64(32)) | (bt - T0).astype(np.uint64)
    o = np.argsort(code, kind="stable")
    code, bv = code[o], bv[o]
    first = np.ones(code.size, bool)
    first[1:] = code[1:] != code[:-1]
    at = np.flatnonzero(first)
    agg = np.add.reduceat(bv, at) if op == "sum" else np.maximum.reduceat(bv, at)
    ucode = code[at]
    old = (keys[keep] << np.uint64(32)) | (times[keep] - T0).astype(np.uint64)
    pos = np.searchsorted(old, ucode)
    nk = np.insert(keys[keep], pos, ucode >> np.uint64(32))
    nt = np.insert(times[keep], pos, (ucode & np.uint64(0xFFFFFFFF)).astype(np.int64) + T0)
    nv = np.insert(vals[keep], pos, agg)
    nln = np.bincount(nk.astype(np.int64), minlength=K).astype(np.uint64)
    hist = nv[np.lexsort((nv, nk))]
    mom = dict(mom)
    mom["n"] = nln.astype(mom["n"].dtype)
    t2 = time.perf_counter()
    st.load(mom)
    st.load_history(nln, hist)
    st.load_series(nln, nv)
    st.load_times(nt)
    t3 = time.perf_counter()
    return {"export_s": t1 - t0, "numpy_s": t2 - t1, "import_s": t3 - t2, "total_s": t3 - t0}


def run_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    seed = args.seed + K
    st = eng.state_create(K, history=True, series=True, times=True)
    twin = eng.state_create(K, history=True, series=True, times=True)
    last = None
    for h in range(HOURS):
        rows = hour(K, step, args.rows, seed, h)
        d = tuple(DeviceArray.from_host(eng, x) for x in rows)
        for s in (st, twin):
            eng.run_stream(s, *d, agg_flow=agg, value_op=op).close()
        for x in d:
            x.free()
        last = rows
    end = T0 + HOURS * HOUR
    out = {"keys": K, "step_s": step, "op": op, "series_points": st.series_points(), "state_bytes": st.nbytes(), "rereads": {}}
    for label, span in REREADS.items():
        from_t = end - span
        sel = last[1] >= from_t
        batch = tuple(x[sel] for x in last)
        d = tuple(DeviceArray.from_host(eng, x) for x in batch)
        rec = {"replace_ms": [], "replace_wall_ms": [], "merge_ms": [], "merge_wall_ms": [], "host": []}
        for r in range(args.reps):
            t = time.perf_counter()
            a = eng.replace_stream(st, *d, from_t=from_t, to_t=end, ranged=True, agg_flow=agg, value_op=op)
            rec["replace_wall_ms"].append((time.perf_counter() - t) * 1e3)
            rec["replace_ms"].append(a["ms_total"])
            t = time.perf_counter()
            b = eng.merge_stream(twin, *d, agg_flow=agg, value_op="max")
            rec["merge_wall_ms"].append((time.perf_counter() - t) * 1e3)
            rec["merge_ms"].append(b["ms_total"])
            if r < args.host_reps:
                rec["host"].append(host_change(st, batch, from_t, end, op))
        for x in d:
            x.free()
        ra, rb = median_after_first(rec["replace_ms"]), median_after_first(rec["merge_ms"])
        host = median_after_first([h["total_s"] for h in rec["host"]]) * 1e3 if rec["host"] else None
        out["rereads"][label] = {
            "batch_rows": int(batch[0].size), "batch_points": int(a["batch_points"]), "points_replaced": int(a["points_replaced"]),
            "points_erased": int(a["points_erased"]), "points_combined_by_the_merge": int(b["points_combined"]),
            "keys_replayed": int(a["keys_replayed"]), "replace_ms_median": ra, "merge_ms_median": rb, "replace_over_merge": ra / rb if rb else None,
            "replace_wall_ms_median": median_after_first(rec["replace_wall_ms"]), "merge_wall_ms_median": median_after_first(rec["merge_wall_ms"]),
            "replace_stage0_ms": a["ms_stage0"], "replace_after_stage0_ms": a["ms_replace"], "merge_stage0_ms": b["ms_stage0"], "merge_after_stage0_ms": b["ms_merge"],
            "host_export_numpy_import_ms_median": host, "host_phases_s": rec["host"], **{k: rec[k] for k in ("replace_ms", "merge_ms")}}
        print("# %s %s: replace %.3f ms, merge(max) %.3f ms, ratio %.2f, host %s ms (%d points replaced)" % (
            name, label, ra, rb, ra / rb if rb else float("nan"), "%.0f" % host if host is not None else "-", a["points_replaced"]), file=sys.stderr, flush=True)
    st.close()
    twin.close()
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_replace", "rows_per_day": args.rows, "hours": HOURS, "reps": args.reps, "host_reps": args.host_reps, "shapes": {}}
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
