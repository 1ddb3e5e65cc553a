#!/usr/bin/env python3
"""Timing of tad_run_state — the batch verdicts of a streaming state's whole window, from the state alone — against the alternative a
caller has without it: tad_run over W, the table with one row per series point the state holds, in device columns.

Shapes: the two of tools/stream_trim_bench.py at their full 24 h window (1e8 rows a day in hourly batches, generated on the device):
  svc   -- 1e5 keys at minute resolution, `sum`  (about 7.2e7 points);
  conn  -- 1e6 connection keys at second resolution, `max`  (about 1e8 points);
both on a state with history, series and times (flags 11), for EWMA and DBSCAN; and
  arima -- the C3 layout (1e8 rows, 1e5 keys, 250 one-minute buckets, 25 batches of 10 buckets) on a series + times state (flags 10)
           trimmed to the newest --keep-points points of every key before every batch, for ARIMA.
Protocol: one engine; (a) tad_run_state and (b) tad_run over W alternate, --reps times each (default 12) after one untimed pair whose
rows are compared bit for bit ("identical"); the figure is tad_stats.ms_total (device events), median with min / max; wall time beside it.
`walk_bytes`: what the EWMA walks have to move, computed from the shape — count and emit walk 8 B per point and 32 B per key each, the
staged emit 56 B more per row (time and value re-read, five columns written) — to be divided by the k_win_ewma<false, false> /
k_win_emit_staged times of a `rocprofv3 --kernel-trace --stats` run of its own (profiles/stream_window_kernel_stats.csv).
Prints one JSON line (profiles/stream_window_bench.json).
usage: python tools/stream_window_bench.py [--rows N] [--shapes svc,conn,arima] [--hours H] [--keep-points P] [--reps R] [--no-check]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn,arima")
ap.add_argument("--hours", type=int, default=24)
ap.add_argument("--keep-points", type=int, default=100)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--no-check", action="store_true")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")
DEV = torch.device("cuda:0")


def hour(K, step, rows, seed, h):
    """the rows of hour h (device), in arbitrary order: every key's values around a base of its own, one in 1e3 a spike"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed * 1000 + h)
    n = rows // 24 + (1 if h % 24 < rows % 24 else 0)
    k = torch.randint(0, K, (n,), generator=g, device=DEV, dtype=torch.int64)
    t = T0 + h * HOUR + step * torch.randint(0, HOUR // step, (n,), generator=g, device=DEV, dtype=torch.int64)
    v = 1_000_000 + (k * 2654435761) % (1 << 30) + torch.randint(0, 1 << 20, (n,), generator=g, device=DEV, dtype=torch.int64)
    v = torch.where(torch.rand(n, generator=g, device=DEV) < 1e-3, v * 5, v)
    return k, t, v


def window_columns(st):
    """W in device columns: one row per series point, (key, time, value)"""
    ln, vals = st.export_series()
    t = st.export_times()
    k = torch.repeat_interleave(torch.arange(st.num_keys, device=DEV, dtype=torch.int64), torch.from_numpy(ln.astype(np.int64)).to(DEV))
    cols = (k.contiguous(), torch.from_numpy(t).to(DEV), torch.from_numpy(vals.view(np.int64)).to(DEV))
    torch.cuda.synchronize()
    return cols


def same(a, b):
    ah, bh = a.to_host(), b.to_host()
    return a.n_rows == b.n_rows and all(np.array_equal(np.asarray(ah[f]).view(np.uint64), np.asarray(bh[f]).view(np.uint64)) for f in FIELDS)


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def measure(eng, st, W, K, algo, **kw):
    """(a) tad_run_state against (b) tad_run over W, alternating"""
    def a():
        return eng.run_state(st, algo=algo, out="device", **kw)

    def b():
        return eng.run(algo, W[0], W[1], W[2], K, agg_flow="svc", value_op="sum", out="device", **kw)

    ra, rb = a(), b()        # warm-up of both; the rows compared before anything is timed
    rec = {"points": ra.stats["n_points"], "keys": ra.stats["n_keys"], "rows": ra.n_rows, "b_stage0_path": rb.stats["stage0_path"],
           "identical": None if args.no_check else bool(same(ra, rb))}
    ra.close()
    rb.close()
    ms = {"a": [], "b": []}
    wall = {"a": [], "b": []}
    b_stage0 = []
    for _ in range(args.reps):
        for name, fn in (("a", a), ("b", b)):
            t = time.perf_counter()
            r = fn()
            wall[name].append((time.perf_counter() - t) * 1e3)
            ms[name].append(r.stats["ms_total"])
            if name == "b":
                b_stage0.append(r.stats["ms_meta"] + r.stats["ms_stage0"])
            r.close()
    rec.update({"run_state_ms": spread(ms["a"]), "tad_run_ms": spread(ms["b"]), "run_state_wall_ms": spread(wall["a"]),
                "tad_run_wall_ms": spread(wall["b"]), "tad_run_stage0_ms": spread(b_stage0),
                "faster": statistics.median(ms["a"]) < statistics.median(ms["b"])})
    print("# %s: tad_run_state %.3f ms (%.3f - %.3f), tad_run over W %.3f ms (%.3f - %.3f, Stage 0 %.3f), %d points, %d rows, identical %s" % (
        algo, rec["run_state_ms"]["median"], rec["run_state_ms"]["min"], rec["run_state_ms"]["max"], rec["tad_run_ms"]["median"],
        rec["tad_run_ms"]["min"], rec["tad_run_ms"]["max"], rec["tad_run_stage0_ms"]["median"], rec["points"], rec["rows"], rec["identical"]),
        file=sys.stderr, flush=True)
    return rec


def run_window(eng, name):
    K, step, agg, op = SHAPES[name]
    st = eng.state_create(K, history=True, series=True, times=True)
    for h in range(args.hours):
        eng.run_stream(st, *hour(K, step, args.rows, args.seed + K, h), agg_flow=agg, value_op=op).close()
    P = st.series_points()
    print("# %s: %d hours streamed, %d points, %.2f GB of state" % (name, args.hours, P, st.nbytes() / 1e9), file=sys.stderr, flush=True)
    W = window_columns(st)
    rec = {"keys": K, "step_s": step, "op": op, "hours": args.hours, "points": P, "state_bytes": st.nbytes(),
           "walk_bytes": {"count": 8 * P + 32 * K, "emit_walk": 8 * P + 32 * K, "emit_per_row": 56}}
    for algo in ("EWMA", "DBSCAN"):
        rec[algo] = measure(eng, st, W, K, algo)
    st.close()
    return rec


def run_arima(eng):
    K, T, WB, STEP = 100_000, 250, 10, 60
    nb = (T + WB - 1) // WB
    cols = [torch.empty(args.rows, dtype=torch.int64, device=DEV) for _ in range(3)]
    eng.synth(0, args.rows, K, T, into=cols)
    order = torch.argsort((cols[1] - T0) // STEP, stable=True)
    k, t, v = (c[order].contiguous() for c in cols)
    del cols, order
    bucket = (t - T0) // STEP
    ends = [int(x) for x in torch.searchsorted(bucket, torch.arange(WB, T + WB, WB, device=DEV)).cpu()]
    starts = [0] + ends[:-1]
    del bucket
    torch.cuda.synchronize()
    st = eng.state_create(K, series=True, times=True)
    for b in range(nb):       # (EWMA batches: the series and its times are what the window call reads)
        st.trim(keep_points=args.keep_points)
        eng.run_stream(st, k[starts[b]:ends[b]], t[starts[b]:ends[b]], v[starts[b]:ends[b]], agg_flow="svc").close()
    st.trim(keep_points=args.keep_points)
    del k, t, v
    P = st.series_points()
    print("# arima: %d batches streamed, %d points" % (nb, P), file=sys.stderr, flush=True)
    W = window_columns(st)
    rec = {"keys": K, "buckets": T, "batches": nb, "keep_points": args.keep_points, "points": P, "ARIMA": measure(eng, st, W, K, "ARIMA")}
    m = rec["ARIMA"]
    m["stage0_share_of_tad_run"] = m["tad_run_stage0_ms"]["median"] / m["tad_run_ms"]["median"]
    st.close()
    return rec


def main():
    eng = TadEngine(device=0)
    res = {"bench": "stream_window", "rows_per_day": args.rows, "reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_arima(eng) if name == "arima" else run_window(eng, name)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
