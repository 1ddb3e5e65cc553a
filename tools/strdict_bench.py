"""tad_strdict against tad_encode_strings and the host vocabulary it replaces ("A string dictionary that outlives the call").

One MI355X, one engine, the variants in alternating order.  A column of n pod-name-like strings with d distinct values goes through
  (a) tad_strdict_encode on a warm dictionary (every string known), (b) the same on a cold dictionary (created per call),
  (c) tad_encode_strings on the same batch, (d) the previous host vocabulary (np.unique + a Python dict) with its core count,
and StringDict.match is timed against the Python mask loop.  Every call ends in a host synchronisation, so the wall clock around a call
on device-resident columns is the call; median and range of `--reps` calls after a warm-up.  Writes profiles/strdict_bench.json.  No gate
on any ratio; the claim to read off is whether (a) stays inside the run-to-run range of (c) or below it.

    python tools/strdict_bench.py [--rows 10000000] [--distinct 1000,100000,10000000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theia_amd import TadEngine, _capi as capi      # noqa: E402
from theia_amd.engine import DeviceArray          # noqa: E402


def pod_names(distinct, rows, rng):
    """`rows` picks from `distinct` names like "coredns-5d78c9869d-x7k2p-000123" as (offsets int32, data uint8, list of str)"""
    hexd = np.array(list("0123456789abcdef"))
    names = ["%s-%s-%07d" % (("coredns", "antrea-agent", "kube-proxy", "theia-manager")[i % 4], "".join(rng.choice(hexd, 10)), i) for i in range(distinct)]
    raw = np.array([s.encode() for s in names], dtype=object)
    pick = rng.integers(0, distinct, rows)
    lens = np.fromiter((len(r) for r in raw), dtype=np.int64, count=distinct)[pick]
    off = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(raw[pick].tolist()), dtype=np.uint8)
    return off, data, names, pick


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": reps}


def host_vocabulary(strings):
    code, values = {}, []
    uniq, inv = np.unique(strings, return_inverse=True)
    codes = np.empty(uniq.size, dtype=np.int64)
    for i, s in enumerate(uniq.tolist()):
        c = code.get(s)
        if c is None:
            c = code[s] = len(values)
            values.append(s)
        codes[i] = c
    return codes[inv]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--distinct", default="1000,100000,10000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=1_000_000, help="rows of the host vocabulary's batch (it is timed once)")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    out = {"rows": args.rows, "cores": os.cpu_count(), "encode": [], "match": []}
    with TadEngine(device=0) as eng:
        for distinct in [int(x) for x in args.distinct.split(",")]:
            off, data, names, pick = pod_names(distinct, args.rows, rng)
            col = (DeviceArray.from_host(eng, off), DeviceArray.from_host(eng, data))
            warm = eng.string_dict()
            warm.encode(col, out="device")

            def cold():
                d = eng.string_dict()
                d.encode(col, out="device")
                d.close()
            res = {"distinct": distinct}
            for _ in range(2):      # alternating order: the second round's numbers are kept
                res["a_warm_strdict"] = timed(lambda: warm.encode(col, out="device"), args.reps)
                res["c_encode_strings"] = timed(lambda: eng.encode_strings(col), args.reps)
                res["b_cold_strdict"] = timed(cold, max(args.reps // 4, 3), warm=1)
            ra, rc = res["a_warm_strdict"], res["c_encode_strings"]
            res["a_inside_or_below_range_of_c"] = bool(ra["median_ms"] <= rc["max_ms"])
            host_strings = np.array(names, dtype=str)[pick[:args.host_rows]]
            t = time.perf_counter()
            host_vocabulary(host_strings)
            res["d_host_vocabulary"] = {"rows": int(host_strings.size), "ms": (time.perf_counter() - t) * 1e3}
            out["encode"].append(res)
            if distinct >= 100000:
                m = {"values": warm.num_values()}
                for op, pat in ((capi.TAD_STR_EQUAL, names[7]), (capi.TAD_STR_CONTAINS_NOCASE, "Proxy-")):
                    m["device_op%d" % op] = timed(lambda: warm.match(op, pat, out="device"), args.reps)
                    t = time.perf_counter()
                    p = pat.lower()
                    np.fromiter((1 if ((s == pat) if op == capi.TAD_STR_EQUAL else (p in s.lower())) else 0 for s in names), dtype=np.uint8, count=len(names))
                    m["host_op%d_ms" % op] = (time.perf_counter() - t) * 1e3
                out["match"].append(m)
            warm.close()
            print(json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "strdict_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["match"]))


if __name__ == "__main__":
    main()
