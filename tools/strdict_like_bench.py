"""tad_strdict_like against the case-folded substring search and the host regex it replaces ("LIKE patterns on the device").

One MI355X, one engine, the variants in alternating order.  A dictionary of n label-set strings of 60 - 120 bytes goes through
  (a) StringDict.like('%lit%', nocase=True), (b) StringDict.match(TAD_STR_CONTAINS_NOCASE, lit) — the reference point, not the code under
  test: a wildcard-free label keeps going through (b) —, (c) StringDict.like with a _ pattern ('%"test_key":"test_value"%'),
and (c) is held against what it replaces: the export of every label string to the host and the batch job's regex over them, timed once on
at most --host-values values.  Every call ends in a host synchronisation and writes a device mask, so the wall clock around a call is the
call; median and range of `--reps` calls after a warm-up.  Writes profiles/strdict_like_bench.json.  No gate on any ratio.

    python tools/strdict_like_bench.py [--values 1000000,10000000] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from theia_amd import TadEngine, _capi as capi                     # noqa: E402
from theia_amd import anomaly_detection as ad                      # noqa: E402
from theia_amd.engine import DeviceArray                           # noqa: E402

LIT = '"app":"db"'
WILD = '"test_key":"test_value"'


def label_sets(n, rng):
    """n distinct label-set strings of 60 - 120 bytes as (offsets int64, data uint8, bytes of all): a tenth carry "app":"db", a twentieth
    "test_key":"test_value", another twentieth "testXkey":"test-value" (the _ matches it)"""
    apps = ("web", "db", "cache", "dns", "api", "worker", "ingest", "front", "queue", "auth")
    extra = ("", ',"test_key":"test_value"', "", ',"testXkey":"test-value"') + ("",) * 16
    pad = rng.integers(5, 50, n)
    raw = [('{"app":"%s","pod-template-hash":"%010x"%s,"zone":"%s"}' % (apps[i % 10], i, extra[i % 20], "z" * int(pad[i]))).encode() for i in range(n)]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(r) for r in raw), dtype=np.int64, count=n), out=off[1:])
    return off, np.frombuffer(b"".join(raw), dtype=np.uint8), raw


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-values", type=int, default=1_000_000, help="values of the host export + regex (it is timed once)")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    out = {"cores": os.cpu_count(), "literal": LIT, "wildcard": WILD, "runs": []}
    with TadEngine(device=0) as eng:
        for n in [int(x) for x in args.values.split(",")]:
            off, data, raw = label_sets(n, rng)
            d = eng.string_dict(n, int(off[-1]) + 16 * n)
            d.encode((DeviceArray.from_host(eng, off), DeviceArray.from_host(eng, data)), out="device")
            assert d.num_values() == n
            res = {"values": n, "mean_bytes": float(off[-1]) / n}

            def run(fn):
                m, hit = fn()
                base = m._base
                m.free()
                if base is not None:
                    base.free()
                return hit
            a = lambda: run(lambda: d.like("%" + LIT + "%", nocase=True, out="device"))
            b = lambda: run(lambda: d.match(capi.TAD_STR_CONTAINS_NOCASE, LIT, out="device"))
            c = lambda: run(lambda: d.like("%" + WILD + "%", nocase=True, out="device"))
            res["matched"] = {"a": a(), "b": b(), "c": c()}
            assert res["matched"]["a"] == res["matched"]["b"]
            for _ in range(2):      # alternating order: the second round's numbers are kept
                res["a_like_literal"] = timed(a, args.reps)
                res["b_contains_nocase"] = timed(b, args.reps)
                res["c_like_wildcard"] = timed(c, args.reps)
            ra, rb = res["a_like_literal"], res["b_contains_nocase"]
            res["a_inside_range_of_b"] = bool(rb["min_ms"] <= ra["median_ms"] <= rb["max_ms"])
            res["a_over_b_median"] = ra["median_ms"] / rb["median_ms"]
            # what (c) replaces: every label string to a Python list, the regex over them one by one
            hv = min(n, args.host_values)
            t = time.perf_counter()
            labels = d.values(0, hv).to_pylist()
            t_export = time.perf_counter() - t
            rx = ad._like_regex("%" + WILD + "%")
            t = time.perf_counter()
            mask = np.fromiter((1 if rx.match(s) is not None else 0 for s in labels), dtype=np.uint8, count=len(labels))
            t_regex = time.perf_counter() - t
            res["host_export_regex"] = {"values": hv, "export_ms": t_export * 1e3, "regex_ms": t_regex * 1e3, "matched": int(mask.sum())}
            if hv == n:
                assert int(mask.sum()) == res["matched"]["c"]
            out["runs"].append(res)
            d.close()
            print(json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "strdict_like_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
