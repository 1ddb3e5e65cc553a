#!/usr/bin/env python3
"""Timing of tad_keydict_encode against tad_factorize on the same batch, device-resident columns, one engine.

The batch: --rows rows (default 1e7) of 6 key columns.  Dictionaries of --keys keys (default 1e5 and 1e7).  Cases, per dictionary size K:
  a -- every tuple of the batch is known (rows uniform over the K keys);
  b -- 10 % of the rows carry new tuples (uniform over max(K / 10, 1e4) keys the dictionary has never seen);
  c -- batch a into an EMPTY dictionary of the default size (the first batch of a stream).
Yardstick: tad_factorize on the same batch alone — what a caller had for one batch before the dictionary; it does NOT give ids that are
stable from batch to batch, so this is a price comparison, not an alternative.  Both calls are made through ctypes on preallocated device
buffers and timed on the host's clock around the call (each call synchronises before it returns); the order alternates
(dictionary, factorize, dictionary, ...) in one process, --reps times.  Before every timed call of b and c the dictionary is put back
(b: a fresh dictionary filled by tad_keydict_import from the snapshot, untimed; c: a fresh empty one).
Host alternative, on --host-rows rows (default 1e6) of batch b at the first K: a Python dict over the row tuples, incrementally, and
pandas (MultiIndex.factorize of the batch + a merge with the known keys' frame).
Prints one JSON line: rows/s (median, min, max) per case and the ratio of the medians to tad_factorize.
--profile a|b|c: prepare, run exactly ONE timed dictionary call of that case at the first K and exit (for `rocprofv3 --kernel-trace --stats --`).
usage: python tools/keydict_bench.py [--rows N] [--keys K1,K2] [--reps R] [--host-rows N] [--profile a|b|c]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine, _capi as capi  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--keys", default="100000,10000000")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-rows", type=int, default=1_000_000)
ap.add_argument("--seed", type=int, default=3)
ap.add_argument("--profile", default="")
args = ap.parse_args()
NCOLS = 6


def tuples_of(k):
    """key index -> its six columns (injective: 13 x 7 x k // 91)"""
    k = np.asarray(k, dtype=np.int64)
    return [k % 13, (k % 7) * -977, k // 91, k % 3 + (1 << 40), k % 2, k * 31 % 5]


class Batch:
    """a batch in device columns, its tad_key_columns and preallocated outputs"""

    def __init__(self, eng, kidx):
        self.n = int(kidx.size)
        self.host = [np.ascontiguousarray(c, dtype=np.int64) for c in tuples_of(kidx)]
        self.cols = [DeviceArray.from_host(eng, c) for c in self.host]
        self.arr = (C.c_void_p * NCOLS)(*[c.ptr for c in self.cols])
        self.kc = capi.KeyColumns(n_rows=self.n, n_cols=NCOLS, cols_a=self.arr, keep_a=None, cols_b=None, keep_b=None, memory=capi.TAD_MEM_DEVICE)
        self.key = DeviceArray(eng, self.n, np.uint64)
        self.first = DeviceArray(eng, self.n, np.uint64)

    def free(self):
        for x in self.cols + [self.key, self.first]:
            x.free()


def timed_encode(eng, d, b):
    before, after = capi.u64(), capi.u64()
    t0 = time.perf_counter()
    rc = eng._lib.tad_keydict_encode(eng._h, d._h, C.byref(b.kc), b.key.ptr, None, b.first.ptr, b.n, C.byref(before), C.byref(after))
    dt = time.perf_counter() - t0
    eng._check(rc)
    return dt, int(before.value), int(after.value)


def timed_factorize(eng, b):
    nk = capi.u64()
    t0 = time.perf_counter()
    rc = eng._lib.tad_factorize(eng._h, C.byref(b.kc), b.key.ptr, None, b.first.ptr, b.n, C.byref(nk))
    dt = time.perf_counter() - t0
    eng._check(rc)
    return dt, int(nk.value)


def summary(secs, rows):
    r = rows / np.asarray(secs)
    return {"rows_per_s": float(np.median(r)), "min": float(r.min()), "max": float(r.max()), "ms": float(np.median(secs) * 1e3), "n": len(secs)}


def host_alternative(K, kidx):
    """the incremental tuple -> id map of a streaming host, on the first --host-rows rows of batch b"""
    import pandas as pd
    kidx = kidx[:args.host_rows]
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in tuples_of(kidx)]
    known = dict((t, i) for i, t in enumerate(zip(*[c.tolist() for c in tuples_of(np.arange(K))])))
    t0 = time.perf_counter()
    ids = np.empty(kidx.size, dtype=np.uint64)
    for i, t in enumerate(zip(*[c.tolist() for c in cols])):
        j = known.get(t)
        if j is None:
            j = known[t] = len(known)
        ids[i] = j
    t_dict = time.perf_counter() - t0
    names = ["c%d" % c for c in range(NCOLS)]
    frame = pd.DataFrame(dict(zip(names, tuples_of(np.arange(K)))))
    frame["id"] = np.arange(K)
    t0 = time.perf_counter()
    batch = pd.DataFrame(dict(zip(names, cols)))
    codes, uniq = pd.MultiIndex.from_frame(batch).factorize()
    u = pd.DataFrame({nm: uniq.get_level_values(i) for i, nm in enumerate(names)}).merge(frame, how="left", on=names)
    new = u["id"].isna().to_numpy()
    u.loc[new, "id"] = K + np.arange(int(new.sum()))
    ids2 = u["id"].to_numpy().astype(np.uint64)[codes]
    t_pandas = time.perf_counter() - t0
    assert np.array_equal(ids, ids2)
    return {"rows": int(kidx.size), "python_dict_rows_per_s": kidx.size / t_dict, "pandas_rows_per_s": kidx.size / t_pandas}


def run_size(eng, K, want_host):
    rng = np.random.default_rng(args.seed + K)
    n = args.rows
    k_a = rng.integers(0, K, size=n)
    n_new_keys = max(K // 10, 10_000)
    k_b = np.where(rng.random(n) < 0.1, K + rng.integers(0, n_new_keys, size=n), rng.integers(0, K, size=n))
    # the dictionary of K keys, and its snapshot (case b puts it back before every timed call)
    seed_batch = Batch(eng, np.arange(K))
    d = eng.key_dict(NCOLS)
    timed_encode(eng, d, seed_batch)
    seed_batch.free()
    assert d.num_keys() == K
    snap = d.export()
    batch_a, batch_b = Batch(eng, k_a), Batch(eng, k_b)
    out = {"keys": K, "rows": n, "dictionary_bytes": d.nbytes()}

    def restored():
        r = eng.key_dict(NCOLS)
        r.load(*snap)
        return r

    def case_a():
        return timed_encode(eng, d, batch_a)

    def case_b():
        r = restored()
        res = timed_encode(eng, r, batch_b)
        r.close()
        return res

    def case_c():
        r = eng.key_dict(NCOLS)
        res = timed_encode(eng, r, batch_a)
        r.close()
        return res

    cases = {"a": (case_a, batch_a), "b": (case_b, batch_b), "c": (case_c, batch_a)}
    if args.profile:
        dt, before, after = cases[args.profile][0]()
        print("# profile %s at %d keys: %.3f ms, %d -> %d keys" % (args.profile, K, dt * 1e3, before, after), file=sys.stderr, flush=True)
        return {"keys": K, "profile": args.profile, "ms": dt * 1e3}
    # the ids of the dictionary against tad_factorize's, before anything is timed: the same partition of the rows
    for name, (fn, b) in cases.items():
        dt, before, after = fn()
        ids = b.key.to_host()
        _, nk = timed_factorize(eng, b)
        fz = b.key.to_host()
        to_dict = np.zeros(nk, dtype=np.uint64)
        to_dict[fz] = ids                      # factorize id -> dictionary id is a function, onto as many ids as there are keys in the batch
        out[name] = {"keys_before": before, "new_keys": after - before, "distinct_in_batch": nk,
                     "same_partition_as_factorize": bool(np.array_equal(to_dict[fz], ids) and np.unique(ids).size == nk), "dict": [], "factorize": []}
        print("# %d keys, case %s: %s" % (K, name, {k: v for k, v in out[name].items() if not isinstance(v, list)}), file=sys.stderr, flush=True)
    for _ in range(args.reps):
        for name, (fn, b) in cases.items():
            out[name]["dict"].append(fn()[0])
            out[name]["factorize"].append(timed_factorize(eng, b)[0])
    for name in cases:
        rec = out[name]
        rec["dict"], rec["factorize"] = summary(rec["dict"], n), summary(rec["factorize"], n)
        rec["time_vs_factorize"] = rec["dict"]["ms"] / rec["factorize"]["ms"]
        print("# %d keys, case %s: dictionary %.3g rows/s (%.2f ms), tad_factorize %.3g rows/s (%.2f ms), time ratio %.2f" % (
            K, name, rec["dict"]["rows_per_s"], rec["dict"]["ms"], rec["factorize"]["rows_per_s"], rec["factorize"]["ms"], rec["time_vs_factorize"]),
            file=sys.stderr, flush=True)
    if want_host:
        out["host_alternative"] = host_alternative(K, k_b)
        print("# host alternative: %s" % out["host_alternative"], file=sys.stderr, flush=True)
    batch_a.free(), batch_b.free()
    d.close()
    return out


def main():
    eng = TadEngine(device=0)
    res = {"bench": "keydict", "rows": args.rows, "key_columns": NCOLS, "reps": args.reps, "results": []}
    sizes = [int(x) for x in args.keys.split(",")]
    for i, K in enumerate(sizes[:1] if args.profile else sizes):
        res["results"].append(run_size(eng, K, want_host=(i == 0 and not args.profile and args.host_rows > 0)))
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
