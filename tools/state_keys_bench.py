#!/usr/bin/env python3
"""Timing of tad_run_state_keys — a job over selected keys of a streaming state — against what a host does without it: tad_run_state_window
over every key, then the rows of the selected keys filtered on the host.  The baseline needs no new call.

States: 24 h of tools/state_window_bench.py's two shapes (1e8 rows a day in hourly batches, generated on the device), history + series +
times:
  svc   -- 1e5 keys at minute resolution, `sum`;
  conn  -- 1e6 connection keys at second resolution, `max`.
Per state, for EWMA and DBSCAN over the whole 24 h and for ARIMA over the newest --keep-points points of every key (svc only: the fits
are proportional to the points judged), at selected shares 1e-4, 1e-2, 0.5 and 1 of the keys (a seeded random mask, in device memory):
  (a) keys      tad_run_state_keys with the mask;
  (b) window    tad_run_state_window with the same window, plus `filter_host_ms`: the wall time of copying its rows to the host and
                keeping those of the selected keys (numpy), which (a) does not need.
Protocol: one engine; one untimed pair whose rows are compared bit for bit after the host filter ("identical"); then (a) and (b)
alternate, --reps times each (default 20); the figure is tad_stats.ms_total (device events), median with min / max.  `mask_free`: at
share 1, whether (a)'s median lies inside (b)'s min .. max — the mask costs nothing when it selects everything.
Also tad_keydict_select at 1e5 and 1e7 keys (three key columns, two terms, masks and output in device memory; wall time around the
call, which synchronises once) against the same rule in numpy on the exported tuples.
Prints one JSON line (profiles/state_keys_bench.json).
usage: python tools/state_keys_bench.py [--rows N] [--shapes svc,conn] [--detectors EWMA,DBSCAN,ARIMA] [--hours H] [--keep-points P]
                                        [--reps R] [--select-keys 100000,10000000] [--no-check]"""
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
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn")
ap.add_argument("--detectors", default="EWMA,DBSCAN,ARIMA")
ap.add_argument("--hours", type=int, default=24)
ap.add_argument("--keep-points", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--select-keys", default="100000,10000000")
ap.add_argument("--no-check", action="store_true")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
SHAPES = {"svc": (100_000, 60, "svc", "sum"), "conn": (1_000_000, 1, "", "max")}   # keys, time step, agg_flow, op
SHARES = (1e-4, 1e-2, 0.5, 1.0)
FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")
DEV = torch.device("cuda:0")
DETECTORS = tuple(args.detectors.split(","))


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


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def device_bytes(eng, a):
    """a uint8 numpy array as a DeviceArray of bytes"""
    pad = np.concatenate([a, np.zeros(-a.size % 8, np.uint8)]) if a.size % 8 or a.size == 0 else a
    return DeviceArray.from_host(eng, np.ascontiguousarray(pad).view(np.uint64)).view(0, a.size, np.uint8)


def filtered(res, keep):
    """the host's filter of (b): the rows to the host, those of the selected keys kept"""
    t = time.perf_counter()
    host = res.to_host()
    sel = keep[host["key_id"].astype(np.int64)] != 0
    rows = {f: np.asarray(host[f])[sel] for f in FIELDS}
    return rows, (time.perf_counter() - t) * 1e3


def measure(eng, st, K, algo, share, win):
    rng = np.random.default_rng(args.seed + int(share * 1e6))
    keep = np.ones(K, np.uint8) if share >= 1.0 else (rng.random(K) < share).astype(np.uint8)
    if not keep.any():
        keep[int(rng.integers(0, K))] = 1
    dkeep = device_bytes(eng, keep)
    kw = {"algo": algo}
    a = lambda: eng.run_state_keys(st, dkeep, *win, **kw)
    b = lambda: eng.run_state_window(st, *win, **kw)
    ra, rb = a(), b()
    rows_b, _ = filtered(rb, keep)
    ha = ra.to_host()
    rec = {"share": share, "keys_selected": int(keep.sum()), "points": ra.stats["n_points"], "points_all": rb.stats["n_points"], "rows": ra.n_rows,
           "rows_all": rb.n_rows, "arima_fits": ra.stats["arima_fits"], "arima_fits_all": rb.stats["arima_fits"],
           "identical": None if args.no_check else bool(ra.n_rows == rows_b["key_id"].size and all(
               np.array_equal(np.asarray(ha[f]).view(np.uint64), rows_b[f].view(np.uint64)) for f in FIELDS))}
    ra.close()
    rb.close()
    ms = {"keys": [], "window": []}
    filt = []
    for _ in range(args.reps):
        r = a()
        ms["keys"].append(r.stats["ms_total"])
        r.close()
        r = b()
        ms["window"].append(r.stats["ms_total"])
        filt.append(filtered(r, keep)[1])
        r.close()
    rec["keys_ms"], rec["window_ms"], rec["filter_host_ms"] = spread(ms["keys"]), spread(ms["window"]), spread(filt)
    x, y = rec["keys_ms"], rec["window_ms"]
    rec["faster"] = x["median"] < y["median"]
    if share >= 1.0:
        rec["mask_free"] = y["min"] <= x["median"] <= y["max"]
    print("#   %s share %g: keys %.3f ms (%.3f - %.3f), window %.3f ms (%.3f - %.3f) + host filter %.3f ms, %d of %d points, identical %s" % (
        algo, share, x["median"], x["min"], x["max"], y["median"], y["min"], y["max"], rec["filter_host_ms"]["median"], rec["points"],
        rec["points_all"], rec["identical"]), file=sys.stderr, flush=True)
    return rec


def run_state_shape(eng, name):
    K, step, agg, op = SHAPES[name]
    st = eng.state_create(K, history=True, series=True, times=True)
    for h in range(args.hours):
        eng.run_stream(st, *hour(K, step, args.rows, args.seed + K, h), agg_flow=agg, value_op=op).close()
    S = st.series_points()
    print("# %s: %d hours streamed, %d points, %.2f GB of state" % (name, args.hours, S, st.nbytes() / 1e9), file=sys.stderr, flush=True)
    rec = {"keys": K, "step_s": step, "op": op, "hours": args.hours, "points": S, "state_bytes": st.nbytes(), "detectors": {}}
    for algo in DETECTORS:
        if algo == "ARIMA" and name != "svc":
            continue
        win = (0, 0, args.keep_points) if algo == "ARIMA" else (0, 0, 0)
        rec["detectors"][algo] = {"window": win, "shares": [measure(eng, st, K, algo, share, win) for share in SHARES]}
    st.close()
    return rec


def run_select(eng, K):
    """tad_keydict_select over K keys of three columns (namespace, name, direction) against numpy on the exported tuples"""
    card = (50, max(K // 20, 1), 2)
    j = torch.arange(K, device=DEV, dtype=torch.int64)
    cols = [(j % card[0]).contiguous(), (j // card[0]).contiguous(), ((j * 7) % 2).contiguous()]      # distinct tuples: (j % 50, j // 50)
    d = eng.key_dict(3, expected_keys=K)
    step = 1 << 22
    for lo in range(0, K, step):
        d.encode([c[lo:lo + step].contiguous() for c in cols])
    assert d.num_keys() == K
    rng = np.random.default_rng(K)
    m0 = (rng.random(card[0]) < 0.3).astype(np.uint8)
    m1 = (rng.random(int(cols[1].max()) + 1) < 0.5).astype(np.uint8)
    terms = [(0, device_bytes(eng, m0)), (1, device_bytes(eng, m1))]
    keep, n_sel = d.select(terms, out="device")
    ex, _ = d.export()
    t = time.perf_counter()
    want = ((m0[ex[0]] != 0) & (m1[ex[1]] != 0)).astype(np.uint8)
    numpy_ms = (time.perf_counter() - t) * 1e3
    identical = bool(np.array_equal(keep.to_host(), want)) and n_sel == int(want.sum())
    ms = []
    for _ in range(args.reps):
        t = time.perf_counter()
        d.select(terms, out="device")
        ms.append((time.perf_counter() - t) * 1e3)
    rec = {"keys": K, "terms": 2, "selected": n_sel, "identical": identical, "select_ms": spread(ms), "numpy_ms": numpy_ms,
           "bytes_model": K * (32 + 2 + 1)}           # a 32-byte record, one byte per term, one byte written (a model, not a measurement)
    print("# select %d keys: %.3f ms (%.3f - %.3f), numpy %.3f ms, identical %s" % (K, rec["select_ms"]["median"], rec["select_ms"]["min"],
                                                                                   rec["select_ms"]["max"], numpy_ms, identical), file=sys.stderr, flush=True)
    d.close()
    return rec


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_keys", "rows_per_day": args.rows, "reps": args.reps, "library": os.path.basename(os.environ.get("TAD_LIBRARY_PATH", "")),
           "shapes": {}, "select": []}
    for name in [s for s in args.shapes.split(",") if s]:
        res["shapes"][name] = run_state_shape(eng, name)
    for K in [int(x) for x in args.select_keys.split(",") if x]:
        res["select"].append(run_select(eng, K))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
