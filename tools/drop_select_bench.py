#!/usr/bin/env python3
"""Timing of the drop job's flow-row query on the device (tad_drop_select) and of the job that starts from it.

One engine on a stream of the caller's, N device-resident flow rows from a seeded generator (two UInt8 action columns, two 8-byte time
columns, six 8-byte code columns: 66 B a row), at selected shares 0, 1e-4, 1e-2, 0.5 and 1.  Per share:
  select   tad_drop_select alone (device columns in, device result out), by device events on the engine's stream around the call — so the
           figure holds both launches, the scan and the host's read of the total between them — after --warmup calls, median with min /
           max over --calls calls;
  job      drop_select -> factorize over the four tuple columns -> run("DROP", value_op="sum"): flow rows to result rows, wall clock;
  numpy    the direct numpy form of the row rule on the same columns in host memory (the columns are copied out first, untimed), wall
           clock, labelled with the cores this process may use;
  model    bytes by DESIGN.md §5's model — (2 + 1/8 + 1/8) N + m (sectors touched) + 56 m, the sectors bounded by 4 x 32 B a selected
           row and by the 33 B a row the columns hold — over the select's median, as a share of the 8 TB/s peak.  A model, not a counter.
One untimed call per share is compared with the numpy form, column by column ("identical").  Prints one JSON line and writes it to
profiles/drop_select_bench.json.
usage: python tools/drop_select_bench.py [--rows N] [--shares 0,1e-4,1e-2,0.5,1] [--calls 20] [--warmup 3] [--no-numpy]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from theia_amd import TadEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=1e8)
ap.add_argument("--shares", default="0,1e-4,1e-2,0.5,1")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed", type=int, default=17)
ap.add_argument("--no-numpy", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_select_bench.json"))
args = ap.parse_args()

DEV = torch.device("cuda:0")
N = int(args.rows)
T0, DAY, DAYS = 1660176000, 86400, 30
N_IP, N_NS, N_POD = 100_000, 64, 50_000
CODES = ("src_ip", "src_pod_ns", "src_pod_name", "dst_ip", "dst_pod_ns", "dst_pod_name")
FIELDS = ("endpoint_kind", "endpoint_ns", "endpoint_name", "direction", "day_s", "count", "row")
PEAK = 8e12


def columns(share, g):
    """the table at this selected share: the code and time columns are shared between the shares, the two action columns are drawn anew"""
    sel = torch.rand(N, generator=g, device=DEV) < share
    side = torch.rand(N, generator=g, device=DEV)
    drop = (2 + (side * 1024).to(torch.int64) % 2).to(torch.uint8)          # 2 or 3
    idle = torch.tensor([0, 1, 4, 255], dtype=torch.uint8, device=DEV)[(side * 4096).to(torch.int64) % 4]
    ia = torch.where(sel & (side < 0.6), drop, idle)                          # both sides drop on a fifth of the selected rows
    ea = torch.where(sel & (side >= 0.4), drop, idle)
    torch.cuda.synchronize()
    return ia.contiguous(), ea.contiguous(), int(sel.sum().item())


def numpy_select(c, ia, ea):
    ing = (ia == 2) | (ia == 3)
    row = np.flatnonzero(ing | (ea == 2) | (ea == 3))
    ing = ing[row]
    pod = np.where(ing, c["dst_pod_name"][row], c["src_pod_name"][row])
    is_pod = pod != 0
    return {"endpoint_kind": is_pod.astype(np.int64), "endpoint_ns": np.where(is_pod, np.where(ing, c["dst_pod_ns"][row], c["src_pod_ns"][row]), 0),
            "endpoint_name": np.where(is_pod, pod, np.where(ing, c["dst_ip"][row], c["src_ip"][row])), "direction": np.where(ing, 0, 1).astype(np.int64),
            "day_s": c["flow_start_s"][row] // DAY * DAY, "count": np.ones(row.size, dtype=np.uint64), "row": row.astype(np.uint64)}


def spread(x):
    return {"median": statistics.median(x), "min": min(x), "max": max(x), "n": len(x)}


def main():
    stream = torch.cuda.Stream(device=DEV)
    eng = TadEngine(device=0, stream=stream.cuda_stream)          # the engine's one context runs on this stream: events on it bracket a call
    g = torch.Generator(device=DEV)
    g.manual_seed(args.seed)
    c = {"src_ip": torch.randint(0, N_IP, (N,), generator=g, device=DEV), "dst_ip": torch.randint(0, N_IP, (N,), generator=g, device=DEV),
         "src_pod_ns": torch.randint(0, N_NS, (N,), generator=g, device=DEV), "dst_pod_ns": torch.randint(0, N_NS, (N,), generator=g, device=DEV),
         "src_pod_name": torch.randint(0, N_POD, (N,), generator=g, device=DEV), "dst_pod_name": torch.randint(0, N_POD, (N,), generator=g, device=DEV),
         "flow_start_s": T0 + torch.randint(0, DAYS * DAY, (N,), generator=g, device=DEV)}
    c["flow_end_s"] = c["flow_start_s"] + 60
    torch.cuda.synchronize()
    host = None if args.no_numpy else {k: v.cpu().numpy() for k, v in c.items()}
    cores = len(os.sched_getaffinity(0))
    res = {"bench": "drop_select", "rows": N, "calls": args.calls, "warmup": args.warmup, "host_cores": cores, "peak_bytes_per_s": PEAK, "shares": {}}
    for text in args.shares.split(","):
        share = float(text)
        ia, ea, m = columns(share, g)

        def select():
            return eng.drop_select(ia, ea, c["flow_start_s"], *[c[k] for k in CODES], flow_end_s=c["flow_end_s"], src_pod_null=0, dst_pod_null=0)

        rec = {"selected": m}
        rows = select()
        assert rows.n_rows == m, (rows.n_rows, m)
        if host is not None:
            hia, hea = ia.cpu().numpy(), ea.cpu().numpy()
            t = time.perf_counter()
            want = numpy_select(host, hia, hea)
            rec["numpy_s"] = time.perf_counter() - t
            got = rows.to_host()
            rec["identical"] = all(np.array_equal(got[f], want[f]) for f in FIELDS)
            del want, got
        rows.close()
        ms = []
        for i in range(args.warmup + args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            r = select()
            b.record(stream)
            b.synchronize()
            r.close()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        rec["select_ms"] = spread(ms)
        model = (2 + 0.25) * N + m * min(4 * 32.0, 33.0 / max(share, 1e-12)) + 56 * m
        rec["model_bytes"] = model
        rec["model_share_of_peak"] = model / (rec["select_ms"]["median"] * 1e-3) / PEAK
        if m:
            t = time.perf_counter()
            rows = select()
            key, _, first = eng.factorize(rows.tuple_columns())
            out = eng.run("DROP", key, rows["day_s"], rows["count"], max(first.n, 1), agg_flow="svc", value_op="sum", out="device")
            rec["job_s"] = time.perf_counter() - t
            rec["job_keys"], rec["job_rows"] = first.n, out.n_rows
            out.close()
            rows.close()
        res["shares"][text] = rec
        print("# share %s: %d of %d rows, select %.3f ms (%.3f - %.3f), model %.2f GB = %.1f %% of peak, job %s s, numpy %s s on %d cores, identical %s" % (
            text, m, N, rec["select_ms"]["median"], rec["select_ms"]["min"], rec["select_ms"]["max"], model / 1e9, 100 * rec["model_share_of_peak"],
            rec.get("job_s"), rec.get("numpy_s"), cores, rec.get("identical")), file=sys.stderr, flush=True)
    eng.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
