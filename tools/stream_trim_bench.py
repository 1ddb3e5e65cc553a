#!/usr/bin/env python3
"""Timing of a trimmed streaming state (tad_state_trim) against the untrimmed stream, device-resident columns.

DBSCAN: the two shapes of tools/stream_dbscan_bench.py (1e8 rows a day in hourly batches):
  svc   -- 1e5 keys at minute resolution, `sum`;
  conn  -- 1e6 connection keys at second resolution, `max`;
for --hours hourly batches (default 72).  The trimmed state (TAD_STATE_HISTORY | SERIES | TIMES) is cut to the last --window hours
(default 24) before every batch once the window is full; its twin (history only, as in stream_dbscan_bench.py) is never trimmed.
ARIMA: the C3 layout of tools/stream_arima_bench.py (1e8 rows, 1e5 keys, 250 one-minute buckets, 25 batches of 10 buckets), the trimmed
state (SERIES, and TIMES for the check) cut to the newest --keep-points points of every key before every batch, against the untrimmed
series state.
Per batch: stream ms (device = tad_stats.ms_total, and wall), trim ms (wall: the call returns when its kernels are done) and state bytes
(tad_state_bytes), for both states.  On the last batch: the trimmed stream's rows against tad_run over the window (the retained points
and the batch), bit for bit ("identical").
Prints one JSON line.  profiles/stream_trim_kernel_stats.csv: `rocprofv3 --kernel-trace --stats -- python tools/stream_trim_bench.py
--shapes svc,conn --hours 26 --no-twin --no-check`, the dispatches from k_trim_keep to k_trim_moments of the one trim per shape that drops
points (hour 26).
usage: python tools/stream_trim_bench.py [--rows N] [--shapes svc,conn,arima] [--hours H] [--window W] [--keep-points P] [--no-twin]
       [--no-check]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn,arima")
ap.add_argument("--hours", type=int, default=72)
ap.add_argument("--window", type=int, default=24)
ap.add_argument("--keep-points", type=int, default=100)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--no-twin", action="store_true")
ap.add_argument("--no-check", action="store_true")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def hour(K, step, rows, seed, h):
    """the rows of hour h (host), in arbitrary order: every key's values around a base of its own, one in 1e3 a spike"""
    rng = np.random.default_rng(seed * 1000 + h)
    n = rows // 24 + (1 if h % 24 < rows % 24 else 0)
    k = rng.integers(0, K, size=n, dtype=np.uint64)
    t = T0 + h * HOUR + step * rng.integers(0, HOUR // step, size=n).astype(np.int64)
    base = 1_000_000 + (k * np.uint64(2654435761)) % np.uint64(1 << 30)
    v = base + rng.integers(0, 1 << 20, size=n).astype(np.uint64)
    v = np.where(rng.random(n) < 1e-3, v * np.uint64(5), v)
    return k, t, v


def codes(k, t):
    return (np.asarray(k, np.uint64) << np.uint64(32)) | (np.asarray(t, np.int64) - T0).astype(np.uint64)


def same_rows(want, sel, got, n_rows):
    return int(sel.sum()) == n_rows and all(np.array_equal(np.asarray(want[f])[sel].view(np.uint64), np.asarray(got[f]).view(np.uint64))
                                            for f in FIELDS)


def run_dbscan(eng, name):
    K, step, agg, op = SHAPES[name]
    seed = args.seed + K
    st = eng.state_create(K, history=True, series=True, times=True)
    twin = None if args.no_twin else eng.state_create(K, history=True)
    rec = {"stream_ms": [], "stream_wall_ms": [], "trim_ms": [], "dropped": [], "bytes": [], "series_points": [], "twin_stream_ms": [],
           "twin_bytes": [], "stage0_path": []}
    for h in range(args.hours):
        d = tuple(DeviceArray.from_host(eng, x) for x in hour(K, step, args.rows, seed, h))
        if h >= args.window:   # keep the last `window` hours: the points at or after the start of hour h - window
            t = time.perf_counter()
            rec["dropped"].append(st.trim(keep_from=T0 + (h - args.window) * HOUR))
            rec["trim_ms"].append((time.perf_counter() - t) * 1e3)
        else:
            rec["dropped"].append(0)
            rec["trim_ms"].append(0.0)
        t = time.perf_counter()
        r = eng.run_stream(st, *d, agg_flow=agg, value_op=op, algo="DBSCAN")
        rec["stream_wall_ms"].append((time.perf_counter() - t) * 1e3)
        rec["stream_ms"].append(r.stats["ms_total"])
        rec["stage0_path"].append(r.stats["stage0_path"])
        rec["bytes"].append(st.nbytes())
        rec["series_points"].append(st.series_points())
        if twin is not None:
            rt = eng.run_stream(twin, *d, agg_flow=agg, value_op=op, algo="DBSCAN")
            rec["twin_stream_ms"].append(rt.stats["ms_total"])
            rec["twin_bytes"].append(twin.nbytes())
            rt.close()
        print("# %s batch %d: stream %.3f ms, trim %.3f ms, %.2f GB%s" % (
            name, h + 1, rec["stream_ms"][-1], rec["trim_ms"][-1], rec["bytes"][-1] / 1e9,
            "" if twin is None else "; untrimmed %.3f ms, %.2f GB" % (rec["twin_stream_ms"][-1], rec["twin_bytes"][-1] / 1e9)),
            file=sys.stderr, flush=True)
        for x in d:
            x.free()
        if h == args.hours - 1 and not args.no_check:   # tad_run over the window: hours h - window .. h
            got = r.to_host()
            lo = max(0, h - args.window)
            hrs = [hour(K, step, args.rows, seed, i) for i in range(lo, h + 1)]
            acc = tuple(DeviceArray.from_host(eng, np.concatenate([x[i] for x in hrs])) for i in range(3))
            t = time.perf_counter()
            b = eng.run("DBSCAN", *acc, K, agg_flow=agg, value_op=op)
            wall = (time.perf_counter() - t) * 1e3
            bh = b.to_host()
            sel = np.isin(codes(bh["key_id"], bh["flow_end_s"]), np.unique(codes(hrs[-1][0], hrs[-1][1])))
            rec["batch_job"] = {"ms": b.stats["ms_total"], "wall_ms": wall, "rows_in": int(acc[0].n), "identical": bool(same_rows(bh, sel, got, r.n_rows))}
            print("# %s last batch: tad_run over the window (%d rows) %.3f ms, identical %s" % (name, acc[0].n, b.stats["ms_total"],
                                                                                               rec["batch_job"]["identical"]), file=sys.stderr, flush=True)
            b.close()
            for x in acc:
                x.free()
        r.close()
    st.close()
    if twin is not None:
        twin.close()
    return {"keys": K, "step_s": step, "op": op, "window_h": args.window, **rec}


def run_arima(eng):
    K, T, W, STEP = 100_000, 250, 10, 60
    nb = (T + W - 1) // W
    dev = torch.device("cuda:0")
    cols = [torch.empty(args.rows, dtype=torch.int64, device=dev) for _ in range(3)]
    eng.synth(0, args.rows, K, T, into=cols)
    order = torch.argsort((cols[1] - T0) // STEP, stable=True)
    k, t, v = (c[order].contiguous() for c in cols)
    del cols, order
    bucket = (t - T0) // STEP
    ends = [int(x) for x in torch.searchsorted(bucket, torch.arange(W, T + W, W, device=dev)).cpu()]
    starts = [0] + ends[:-1]
    del bucket
    torch.cuda.synchronize()
    st = eng.state_create(K, series=True, times=not args.no_check)
    twin = None if args.no_twin else eng.state_create(K, series=True)
    rec = {"stream_ms": [], "stream_wall_ms": [], "trim_ms": [], "dropped": [], "bytes": [], "series_points": [], "twin_stream_ms": [],
           "twin_bytes": []}
    for b in range(nb):
        lo, hi = starts[b], ends[b]
        bk, bt, bv = k[lo:hi], t[lo:hi], v[lo:hi]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec["dropped"].append(st.trim(keep_points=args.keep_points))
        rec["trim_ms"].append((time.perf_counter() - t0) * 1e3)
        check = b == nb - 1 and not args.no_check
        if check:   # the retained points, one row each, for tad_run over the window
            ln, vals = st.export_series()
            ret = (np.repeat(np.arange(K, dtype=np.uint64), ln.astype(np.int64)), st.export_times(), vals)
        t0 = time.perf_counter()
        r = eng.run_stream(st, bk, bt, bv, agg_flow="svc", algo="ARIMA")
        rec["stream_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        rec["stream_ms"].append(r.stats["ms_total"])
        rec["bytes"].append(st.nbytes())
        rec["series_points"].append(st.series_points())
        if twin is not None:
            rt = eng.run_stream(twin, bk, bt, bv, agg_flow="svc", algo="ARIMA")
            rec["twin_stream_ms"].append(rt.stats["ms_total"])
            rec["twin_bytes"].append(twin.nbytes())
            rt.close()
        print("# arima batch %d: stream %.3f ms, trim %.3f ms, %.3f GB%s" % (
            b + 1, rec["stream_ms"][-1], rec["trim_ms"][-1], rec["bytes"][-1] / 1e9,
            "" if twin is None else "; untrimmed %.3f ms, %.3f GB" % (rec["twin_stream_ms"][-1], rec["twin_bytes"][-1] / 1e9)),
            file=sys.stderr, flush=True)
        if check:
            got = r.to_host()
            bh = (bk.cpu().numpy().view(np.uint64), bt.cpu().numpy(), bv.cpu().numpy().view(np.uint64))
            acc = tuple(DeviceArray.from_host(eng, np.concatenate([ret[i], bh[i]])) for i in range(3))
            t0 = time.perf_counter()
            j = eng.run("ARIMA", *acc, K, agg_flow="svc")
            wall = (time.perf_counter() - t0) * 1e3
            jh = j.to_host()
            tb = np.asarray(jh["flow_end_s"])
            sel = (tb >= T0 + STEP * W * b) & (tb < T0 + STEP * W * (b + 1))
            rec["batch_job"] = {"ms": j.stats["ms_total"], "wall_ms": wall, "rows_in": int(acc[0].n), "identical": bool(same_rows(jh, sel, got, r.n_rows))}
            print("# arima last batch: tad_run over the window (%d rows) %.3f ms, identical %s" % (acc[0].n, j.stats["ms_total"],
                                                                                                  rec["batch_job"]["identical"]), file=sys.stderr, flush=True)
            j.close()
            for x in acc:
                x.free()
        r.close()
    st.close()
    if twin is not None:
        twin.close()
    return {"keys": K, "buckets": T, "batches": nb, "keep_points": args.keep_points, **rec}


def main():
    eng = TadEngine(device=0)
    res = {"bench": "stream_trim", "rows_per_day": args.rows, "hours": args.hours, "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_arima(eng) if name == "arima" else run_dbscan(eng, name)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
