#!/usr/bin/env python3
"""Timing of tad_run_state_window — the batch verdicts over a window of a streaming state, read-only — against the alternative a caller
has without it: tad_run over W', the window's points, in device columns (which flatters the alternative: a real caller must build W').

Shapes: the two of tools/stream_window_bench.py at their full 24 h (1e8 rows a day in hourly batches, generated on the device):
  svc   -- 1e5 keys at minute resolution, `sum`;
  conn  -- 1e6 connection keys at second resolution, `max`;
both on a state with history, series and times (flags 11), for EWMA and DBSCAN, with two windows:
  newest_6h          from_t = the start of hour 18 (a quarter of the state: DBSCAN sorts the window's values);
  all_but_newest_1h  to_t = the start of hour 23 (DBSCAN sorts the excluded hour and subtracts it from the history); and
  arima -- the C3 layout of tools/stream_window_bench.py on a series + times state, one window (the newest half of every key's points).
Protocol: one engine; (a) the windowed call and (b) tad_run over W' alternate, --reps times each (default 12) after one untimed pair whose
rows are compared bit for bit ("identical"); the figure is tad_stats.ms_total (device events), median with min / max.
Also per shape: `whole` — a window whose bounds leave every key whole, (t_min, t_max + 1, 0), against tad_run_state, alternating: the
call runs k_win_bounds, two scans and one more host synchronisation and then judges the state's own arrays (`whole_zero`: all three
arguments zero, which returns to tad_run_state's path before the bounds); and
`ewma_copy` — the windowed EWMA call at newest_6h against tad_run_state on the state after tad_state_trim to the same 6 h (measured last:
the trim is destructive): the price of being non-destructive.
`gather_bytes`: k_win_gather's model per window — 32 B per window point, 16 B per packed excluded value on the subtract path — to be
divided by its time in a `rocprofv3 --kernel-trace --stats` run of its own (profiles/state_window_kernel_stats.csv).
Prints one JSON line (profiles/state_window_bench.json).
DBSCAN's two history paths: build the library twice more with tools/build_variants.py (`sort:TAD_WIN_HIST_FORCE=1`,
`subtract:TAD_WIN_HIST_FORCE=2`) and run this tool with TAD_LIBRARY_PATH naming each and `--detectors DBSCAN`; `library` in the output
says which build ran (profiles/state_window_history_paths.json holds the three lines).
usage: python tools/state_window_bench.py [--rows N] [--shapes svc,conn,arima] [--detectors EWMA,DBSCAN] [--hours H] [--keep-points P]
                                          [--reps R] [--no-check]"""
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
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--shapes", default="svc,conn,arima")
ap.add_argument("--detectors", default="EWMA,DBSCAN")
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


def window_columns(st):
    """W in device columns: one row per series point, (key, time, value), in (key, time) order"""
    ln, vals = st.export_series()
    t = st.export_times()
    k = torch.repeat_interleave(torch.arange(st.num_keys, device=DEV, dtype=torch.int64), torch.from_numpy(ln.astype(np.int64)).to(DEV))
    cols = (k.contiguous(), torch.from_numpy(t).to(DEV), torch.from_numpy(vals.view(np.int64)).to(DEV))
    torch.cuda.synchronize()
    return cols


def inside(W, from_t, to_t, keep):
    """W' of W: the three rules of tad_run_state_window, in their order"""
    k, t, _ = W
    m = torch.ones_like(t, dtype=torch.bool)
    if from_t:
        m &= t >= from_t
    if to_t:
        m &= t < to_t
    if keep:
        idx = torch.nonzero(m).squeeze(1)
        kk = k[idx].contiguous()
        from_end = torch.searchsorted(kk, kk, right=True) - torch.arange(kk.numel(), device=DEV)
        m[idx[from_end > keep]] = False
    cols = tuple(c[m].contiguous() for c in W)
    torch.cuda.synchronize()
    return cols


def same(a, b):
    ah, bh = a.to_host(), b.to_host()
    return a.n_rows == b.n_rows and all(np.array_equal(np.asarray(ah[f]).view(np.uint64), np.asarray(bh[f]).view(np.uint64)) for f in FIELDS)


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def alternate(a, b, names):
    """one untimed pair compared bit for bit, then a and b alternating; ms_total of each"""
    ra, rb = a(), b()
    rec = {"points": ra.stats["n_points"], "keys": ra.stats["n_keys"], "rows": ra.n_rows,
           "identical": None if args.no_check else bool(same(ra, rb))}
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
    rec["faster"] = x["median"] < y["median"]
    rec["ranges_overlap"] = x["max"] >= y["min"] and y["max"] >= x["min"]
    print("#   %s %.3f ms (%.3f - %.3f), %s %.3f ms (%.3f - %.3f), %d points, %d rows, identical %s" % (
        names[0], x["median"], x["min"], x["max"], names[1], y["median"], y["min"], y["max"], rec["points"], rec["rows"], rec["identical"]),
        file=sys.stderr, flush=True)
    return rec


def measure(eng, st, W, K, algo, win, **kw):
    """(a) tad_run_state_window against (b) tad_run over W', alternating"""
    Wp = inside(W, *win)
    print("# %s %s:" % (algo, win), file=sys.stderr, flush=True)
    return alternate(lambda: eng.run_state_window(st, *win, algo=algo, out="device", **kw),
                     lambda: eng.run(algo, Wp[0], Wp[1], Wp[2], K, agg_flow="svc", value_op="sum", out="device", **kw), ("window", "tad_run"))


def run_window(eng, name):
    K, step, agg, op = SHAPES[name]
    st = eng.state_create(K, history=True, series=True, times=True)
    for h in range(args.hours):
        eng.run_stream(st, *hour(K, step, args.rows, args.seed + K, h), agg_flow=agg, value_op=op).close()
    S = st.series_points()
    print("# %s: %d hours streamed, %d points, %.2f GB of state" % (name, args.hours, S, st.nbytes() / 1e9), file=sys.stderr, flush=True)
    W = window_columns(st)
    wins = {"newest_6h": (T0 + (args.hours - 6) * HOUR, 0, 0), "all_but_newest_1h": (0, T0 + (args.hours - 1) * HOUR, 0)}
    rec = {"keys": K, "step_s": step, "op": op, "hours": args.hours, "points": S, "state_bytes": st.nbytes(), "windows": {}}
    for wname, win in wins.items():
        w = {"window": win}
        for algo in DETECTORS:
            w[algo] = measure(eng, st, W, K, algo, win)
        P = w[DETECTORS[0]]["points"]
        w["history_by_sort"] = 2 * P <= S
        w["gather_bytes"] = {"EWMA": 32 * P, "DBSCAN": 32 * P + (0 if 2 * P <= S else 16 * (S - P))}
        rec["windows"][wname] = w
    t_min, t_max = int(W[1].min()), int(W[1].max())
    del W
    for name_w, win in (("whole", (t_min, t_max + 1, 0)), ("whole_zero", (0, 0, 0))):
        print("# %s %s:" % (name_w, win), file=sys.stderr, flush=True)
        rec[name_w] = {algo: alternate(lambda: eng.run_state_window(st, *win, algo=algo, out="device"),
                                       lambda: eng.run_state(st, algo=algo, out="device"), ("window", "run_state")) for algo in DETECTORS}
    if "EWMA" not in DETECTORS:
        st.close()
        return rec
    # the price of being non-destructive: the windowed EWMA call against tad_run_state on the state trimmed to the same window
    win = wins["newest_6h"]
    ms_w = []
    for _ in range(args.reps):
        r = eng.run_state_window(st, *win, out="device")
        ms_w.append(r.stats["ms_total"])
        r.close()
    st.trim(keep_from=win[0])
    ms_t = []
    for _ in range(args.reps + 1):
        r = eng.run_state(st, out="device")
        ms_t.append(r.stats["ms_total"])
        r.close()
    rec["ewma_copy"] = {"window_ms": spread(ms_w), "run_state_on_trimmed_ms": spread(ms_t[1:]), "points": st.series_points()}
    print("# EWMA newest 6 h: windowed %.3f ms, tad_run_state on the trimmed state %.3f ms" % (
        rec["ewma_copy"]["window_ms"]["median"], rec["ewma_copy"]["run_state_on_trimmed_ms"]["median"]), file=sys.stderr, flush=True)
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
    for b in range(nb):
        st.trim(keep_points=args.keep_points)
        eng.run_stream(st, k[starts[b]:ends[b]], t[starts[b]:ends[b]], v[starts[b]:ends[b]], agg_flow="svc").close()
    st.trim(keep_points=args.keep_points)
    del k, t, v
    S = st.series_points()
    print("# arima: %d batches streamed, %d points" % (nb, S), file=sys.stderr, flush=True)
    W = window_columns(st)
    win = (0, 0, args.keep_points // 2)
    rec = {"keys": K, "buckets": T, "batches": nb, "keep_points": args.keep_points, "points": S, "window": win,
           "ARIMA": measure(eng, st, W, K, "ARIMA", win)}
    st.close()
    return rec


def main():
    eng = TadEngine(device=0)
    res = {"bench": "state_window", "rows_per_day": args.rows, "reps": args.reps, "library": os.path.basename(os.environ.get("TAD_LIBRARY_PATH", "")),
           "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = run_arima(eng) if name == "arima" else run_window(eng, name)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
