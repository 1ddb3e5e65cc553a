#!/usr/bin/env python3
"""Narrow input columns (tad.h: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32) against 8-byte ones, on ONE engine, device-resident columns.
Jobs alternate between the widths (64, 64), (64, 32) and (32, 32) — key bits, time bits — so that the three variants see the same box
state; every variant runs --steps jobs per shape.  Shapes: C2 (EWMA, 1e8 rows / 1e5 keys / 250 buckets, round robin over --tables
synthetic tables as bench.py does), C4 (DBSCAN, 1e8 rows / 1e6 keys / 100 buckets, `max`), and the second-resolution shape of
tools/sparse_bench.py's scale run (1e8 rows / 1e6 connections, ~33 points each over a day: the sparse Stage 0).  Prints one JSON line
per (shape, width): median / min / max of the whole job (tad_stats.ms_total), ms_stage0, ms_scatter, and whether the result equals the
8-byte run bit for bit.  Kernel times of pass A / pass B: run under `rocprofv3 --kernel-trace --stats` separately.
usage: python tools/narrow_bench.py [--steps 20] [--tables 2] [--shapes c2,c4,sparse] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tables", type=int, default=2)
ap.add_argument("--shapes", default="c2,c4,sparse")
ap.add_argument("--widths", default="64-64,64-32,32-32")
ap.add_argument("--out", default="")
args = ap.parse_args()
WIDTHS = [tuple(int(x) for x in w.split("-")) for w in args.widths.split(",")]
SHAPES = {"c2": dict(algo="EWMA", rows=100_000_000, keys=100_000, buckets=250, agg="svc"),
          "c4": dict(algo="DBSCAN", rows=100_000_000, keys=1_000_000, buckets=100, agg=""),
          "sparse": dict(algo="EWMA", rows=100_000_000, keys=1_000_000, buckets=0, agg="")}


def sparse_table(n, K, seed):
    """Connections with ~33 second-resolution points each, 3 rows per point, starting anywhere in a day (device, torch)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    conn = torch.randint(0, K, (n,), device="cuda", generator=g, dtype=torch.int64)
    start = (conn * 2654435761) % 86400
    t = 1_700_000_000 + start + 5 * torch.randint(0, 33, (n,), device="cuda", generator=g, dtype=torch.int64)
    v = torch.randint(0, 1 << 40, (n,), device="cuda", generator=g, dtype=torch.int64)
    return conn, t, v


def main():
    eng = TadEngine(device=0)
    out = []
    for shape in args.shapes.split(","):
        sh = SHAPES[shape]
        tabs = []
        for i in range(args.tables):
            if sh["buckets"]:
                k = torch.empty(sh["rows"], dtype=torch.int64, device="cuda")
                t, v = torch.empty_like(k), torch.empty_like(k)
                eng.synth(0, sh["rows"], sh["keys"], sh["buckets"], seed=1000 + i, into=(k, t, v))
            else:
                k, t, v = sparse_table(sh["rows"], sh["keys"], 1000 + i)
            assert int(t.max()) < (1 << 32)
            cols = {(64, 64): (k, t), (64, 32): (k, t.to(torch.int32)), (32, 64): (k.to(torch.int32), t), (32, 32): (k.to(torch.int32), t.to(torch.int32))}
            tabs.append(({w: cols[w] for w in WIDTHS}, v))
        torch.cuda.synchronize()

        def job(i, w):
            (cols, v) = tabs[i % len(tabs)]
            kk, tt = cols[w]
            return eng.run(sh["algo"], kk, tt, v, sh["keys"], agg_flow=sh["agg"])

        # bit-identity on every table, then warm-up
        identical = {w: True for w in WIDTHS}
        for i in range(len(tabs)):
            ref = job(i, (64, 64))
            for w in WIDTHS:
                r = job(i, w)
                same = r.n_rows == ref.n_rows and all(np.array_equal(r[f], ref[f]) for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"))
                same = same and r.stats["stage0_path"] == ref.stats["stage0_path"] and r.stats["hist_sampled"] == ref.stats["hist_sampled"]
                identical[w] = identical[w] and same
        for s in range(args.warmup):
            for w in WIDTHS:
                job(s, w)
        rec = {w: [] for w in WIDTHS}
        for s in range(args.steps):
            for w in (WIDTHS if s % 2 == 0 else WIDTHS[::-1]):     # alternating, order flipped every step
                r = job(s, w)
                rec[w].append((r.stats["ms_total"], r.stats["ms_stage0"], r.stats["ms_scatter"], r.stats["stage0_path"]))
        for w in WIDTHS:
            a = np.array([x[:3] for x in rec[w]])
            line = {"shape": shape, "algo": sh["algo"], "key_bits": w[0], "time_bits": w[1], "steps": args.steps,
                    "ms_total_median": float(np.median(a[:, 0])), "ms_total_min": float(a[:, 0].min()), "ms_total_max": float(a[:, 0].max()),
                    "ms_stage0_median": float(np.median(a[:, 1])), "ms_scatter_median": float(np.median(a[:, 2])),
                    "stage0_path": int(rec[w][0][3]), "identical": bool(identical[w])}
            print(json.dumps(line), flush=True)
            out.append(line)
        del tabs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
