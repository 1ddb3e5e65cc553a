#!/usr/bin/env python3
"""Timing of the streaming ARIMA detector (tad_run_stream with TAD_ALGO_ARIMA on a state with a series), device-resident columns.

The C3 table (default 1e8 rows, 1e5 keys, 250 one-minute buckets, `svc`), generated on the device and cut into 25 batches of 10
buckets (the rows sorted by bucket on the device: batches 1..b are a prefix of the sorted columns).  Per batch: the tad_run_stream ARIMA
time (device = tad_stats.ms_total, and wall), its arima_fits and kalman_steps.  At batches 1, 5, 10 and 25 also tad_run ARIMA over the
window so far -- what a caller pays today for the same predictions -- and whether its rows for the batch's points equal the stream's
bit for bit.
--save-before-last PATH: stop before the last batch and save the state (moments + series) and nothing else is timed;
--resume PATH: load that state into a fresh series state and run the last batch alone (for `rocprofv3 --kernel-trace --stats`).
Prints one JSON line.
usage: python tools/stream_arima_bench.py [--rows N] [--keys K] [--save-before-last P | --resume P]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--keys", type=int, default=100_000)
ap.add_argument("--buckets", type=int, default=250)
ap.add_argument("--per-batch", type=int, default=10)
ap.add_argument("--save-before-last", default=None)
ap.add_argument("--resume", default=None)
args = ap.parse_args()

T_BASE, STEP = 1660202814, 60
CHECK = (1, 5, 10, 25)
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")


def main():
    eng = TadEngine(device=0)
    K, T, W = args.keys, args.buckets, args.per_batch
    nb = (T + W - 1) // W
    dev = torch.device("cuda:0")
    cols = [torch.empty(args.rows, dtype=torch.int64, device=dev) for _ in range(3)]
    eng.synth(0, args.rows, K, T, into=cols)
    order = torch.argsort((cols[1] - T_BASE) // STEP, stable=True)
    k, t, v = (c[order].contiguous() for c in cols)
    del cols, order
    bucket = (t - T_BASE) // STEP
    ends = [int(x) for x in torch.searchsorted(bucket, torch.arange(W, T + W, W, device=dev)).cpu()]
    starts = [0] + ends[:-1]
    del bucket
    torch.cuda.synchronize()

    st = eng.state_create(K, series=True)
    first = 0
    if args.resume:
        z = np.load(args.resume)
        st.load({f: z[f] for f in ("n", "avg", "m2", "ewma", "last_t")})
        st.load_series(z["len"], z["values"])
        first = nb - 1
    rec = {"stream_ms": [], "stream_wall_ms": [], "arima_fits": [], "kalman_steps": [], "rows_out": [], "series_points": [], "stage0_path": [],
           "batch_job": {}}
    for b in range(first, nb):
        if args.save_before_last and b == nb - 1:
            s = st.export()
            ln, vals = st.export_series()
            np.savez(args.save_before_last, len=ln, values=vals, **s)
            break
        lo, hi = starts[b], ends[b]
        bk, bt, bv = k[lo:hi], t[lo:hi], v[lo:hi]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = eng.run_stream(st, bk, bt, bv, agg_flow="svc", algo="ARIMA")
        rec["stream_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        rec["stream_ms"].append(r.stats["ms_total"])
        rec["arima_fits"].append(r.stats["arima_fits"])
        rec["kalman_steps"].append(r.stats["kalman_steps"])
        rec["stage0_path"].append(r.stats["stage0_path"])
        rec["rows_out"].append(r.n_rows)
        rec["series_points"].append(st.series_points())
        got = r.to_host()
        print("# batch %d: %d rows in, stream %.3f ms (wall %.3f), %d fits" % (b + 1, hi - lo, rec["stream_ms"][-1], rec["stream_wall_ms"][-1],
                                                                             rec["arima_fits"][-1]), file=sys.stderr, flush=True)
        if b + 1 in CHECK and not args.resume:
            acc = (k[:hi], t[:hi], v[:hi])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            j = eng.run("ARIMA", *acc, K, agg_flow="svc")
            wall = (time.perf_counter() - t0) * 1e3
            jh = j.to_host()
            tb = np.asarray(jh["flow_end_s"])
            sel = (tb >= T_BASE + STEP * W * b) & (tb < T_BASE + STEP * W * (b + 1))
            same = int(sel.sum()) == r.n_rows and all(np.array_equal(np.asarray(jh[f])[sel].view(np.uint64), np.asarray(got[f]).view(np.uint64))
                                                      for f in FIELDS)
            rec["batch_job"][str(b + 1)] = {"ms": j.stats["ms_total"], "wall_ms": wall, "rows_in": hi, "arima_fits": j.stats["arima_fits"],
                                            "kalman_steps": j.stats["kalman_steps"], "identical": bool(same), "stream_ms": rec["stream_ms"][-1]}
            print("# batch %d: tad_run over %d rows %.3f ms (%d fits), identical %s" % (b + 1, hi, j.stats["ms_total"], j.stats["arima_fits"], same),
                  file=sys.stderr, flush=True)
            j.close()
        r.close()
    st.close()
    eng.close()
    res = {"bench": "stream_arima", "rows": args.rows, "keys": K, "buckets": T, "batches": nb, "buckets_per_batch": W, "resume": bool(args.resume),
           "stream_ms_sum": float(sum(rec["stream_ms"])), **rec}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
