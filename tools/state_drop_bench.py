#!/usr/bin/env python3
"""Timing of the drop detector on a streaming state (tad_drop_state / tad_drop_stream) against what a caller has without it.

States, one row per (key, day), generated on the device and streamed into a series + times state in one batch:
  days365  -- 1e5 keys x 365 points;
  days30   -- 1e6 keys x 30 points;
  long     -- 64 keys x 1e5 points (every key takes the wavefront shape).
Per state:
  whole / half  tad_drop_state over the whole state, and over the window that keeps the newer half of the days, against tad_run(DROP)
                over the same points in device columns — the only way to these rows without the call, and one that flatters the
                alternative (a real caller must first build the columns).  One untimed pair is compared bit for bit ("identical"),
                then the two alternate --reps times; the figure is tad_stats.ms_total (device events), median with min / max;
  stream        tad_drop_stream of one more day against tad_run_stream (EWMA) of the same batch on a twin state, alternating, a new day
                per repetition (the first pair untimed): what judging the day costs on top of keeping the state;
  workspace     the model of both sides' job-context workspace in bytes: tad_run(DROP) holds the K x T grid (9 B a cell) and
                k_drop_detect's K x T doubles; tad_drop_state about 29 B per key and 21 B per judged point (key, verdict, rows, offset).
Prints one JSON line.
usage: python tools/state_drop_bench.py [--shapes days365,days30,long] [--reps R] [--no-check]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="days365,days30,long")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--no-check", action="store_true")
args = ap.parse_args()

DAY0 = 19000                  # day numbers as the time column, as theia_amd.drop_detection feeds them
SHAPES = {"days365": (100_000, 365), "days30": (1_000_000, 30), "long": (64, 100_000)}      # keys, days
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")
DEV = torch.device("cuda:0")
KW = dict(agg_flow="svc", value_op="sum")


def days(K, first, n, seed):
    """one row per (key, day) for the days [first, first + n), key-major: counts around a base per key, one in 500 a tenth of it"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed * 100003 + first)
    k = torch.arange(K, device=DEV, dtype=torch.int64).repeat_interleave(n)
    t = (DAY0 + first + torch.arange(n, device=DEV, dtype=torch.int64)).repeat(K)
    v = 10_000 + (k * 2654435761) % (1 << 20) + torch.randint(0, 1 << 12, (K * n,), generator=g, device=DEV, dtype=torch.int64)
    v = torch.where(torch.rand(K * n, generator=g, device=DEV) < 2e-3, v // 10, v)
    torch.cuda.synchronize()
    return k.contiguous(), t.contiguous(), v.contiguous()


def same(a, b):
    ah, bh = a.to_host(), b.to_host()
    return a.n_rows == b.n_rows and all(np.array_equal(np.asarray(ah[f]).view(np.uint64), np.asarray(bh[f]).view(np.uint64)) for f in FIELDS)


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def alternate(a, b, names, check=True):
    ra, rb = a(), b()
    rec = {"points": ra.stats["n_points"], "rows": ra.n_rows, "identical": bool(same(ra, rb)) if check and not args.no_check else None}
    ra.close()
    rb.close()
    ms = {names[0]: [], names[1]: []}
    for _ in range(args.reps):
        for name, fn in zip(names, (a, b)):
            r = fn()
            ms[name].append(r.stats["ms_total"])
            r.close()
    for name in names:
        rec[name + "_ms"] = spread(ms[name])
    x, y = rec[names[0] + "_ms"], rec[names[1] + "_ms"]
    rec["ratio"] = x["median"] / y["median"]
    rec["ranges_overlap"] = x["max"] >= y["min"] and y["max"] >= x["min"]
    print("#   %s %.3f ms (%.3f - %.3f), %s %.3f ms (%.3f - %.3f), ratio %.2f, %d points, %d rows, identical %s" % (
        names[0], x["median"], x["min"], x["max"], names[1], y["median"], y["min"], y["max"], rec["ratio"], rec["points"], rec["rows"],
        rec["identical"]), file=sys.stderr, flush=True)
    return rec


def run_shape(eng, name):
    K, T = SHAPES[name]
    seed = args.seed + K
    W = days(K, 0, T, seed)
    st, twin = (eng.state_create(K, series=True, times=True) for _ in range(2))
    for s in (st, twin):
        eng.run_stream(s, *W, **KW).close()
    print("# %s: %d keys x %d days, %d points, %.2f GB of state" % (name, K, T, st.series_points(), st.nbytes() / 1e9), file=sys.stderr, flush=True)
    rec = {"keys": K, "days": T, "points": K * T, "state_bytes": st.nbytes()}
    print("# whole:", file=sys.stderr, flush=True)
    rec["whole"] = alternate(lambda: eng.drop_state(st, out="device"), lambda: eng.run("DROP", *W, K, out="device", **KW), ("drop_state", "tad_run"))
    half = DAY0 + T // 2
    m = W[1] >= half
    Wh = tuple(c[m].contiguous() for c in W)
    torch.cuda.synchronize()
    print("# half (from day %d):" % (T // 2), file=sys.stderr, flush=True)
    rec["half"] = alternate(lambda: eng.drop_state(st, half, 0, 0, out="device"), lambda: eng.run("DROP", *Wh, K, out="device", **KW), ("drop_state", "tad_run"))
    del Wh, m
    # one more day per repetition: the drop batch on st, the EWMA batch on the twin (other rows: not compared)
    nxt = iter(range(T, T + 2 * args.reps + 4))
    batch = {}

    def drop_day():
        batch["d"] = days(K, next(nxt), 1, seed)
        return eng.drop_stream(st, *batch["d"], out="device", **KW)

    print("# stream (one day):", file=sys.stderr, flush=True)
    rec["stream"] = alternate(drop_day, lambda: eng.run_stream(twin, *batch["d"], out="device", **KW), ("drop_stream", "ewma_stream"), check=False)
    rec["workspace_bytes_model"] = {"tad_run": K * T * (9 + 8), "drop_state": 29 * K + 21 * K * T}
    st.close()
    twin.close()
    return rec


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_drop", "reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_shape(eng, name)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
