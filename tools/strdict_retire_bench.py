#!/usr/bin/env python3
"""Timing of retiring dead strings (tad_keydict_mark_codes + tad_strdict_compact + tad_keydict_recode) against the only remedy a host had
before: export both dictionaries, select in numpy, import into fresh ones ("Retiring dead strings").

Shape: a vocabulary of --values names of 30 bytes ("deployment-0000012345-abcdefgh": two 16-byte words of arena each) and a key dictionary
of --keys two-column keys (a name's code, a number that makes the tuple distinct).  A share --shares of the values survives: the keys use
codes drawn from the survivors, and the survivors' mask is what the mark call accumulates into — a vocabulary shared with columns the
key dictionary does not hold — so that the surviving share does not depend on the number of keys.
One engine, the same data for both sides (both dictionaries restored from one host snapshot before every repetition, not timed):
  (a) the device chain: KeyDict.used_codes(into the survivors' mask) + StringDict.compact + KeyDict.recode, masks and remaps on the device;
  (b) the host round trip, with the calls the library had before: both exports -> numpy selection and renumbering -> a fresh StringDict
      and a fresh KeyDict with both imports;
after a check that (a)'s exports equal (b)'s selection; alternating, --reps each, median (min-max), wall clock.
  (c) the yardstick of the arena copy: tad_strdict_compact's own time (HIP events over the whole call: flags, two scans, records, copy,
      rehash and the round trip for the totals) beside a device-to-device copy of the survivors' padded bytes — WALL CLOCK: twenty
      copies behind each other ended by one 8-byte read-back, the read-back's own time taken off, divided by twenty.  The copy KERNEL's
      own time, and the same copies on the same clock, are in a trace: `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python
      tools/strdict_retire_bench.py --reps 1 --no-baseline`.
Prints one JSON line per shape.
usage: python tools/strdict_retire_bench.py [--values N,N] [--shares S,S] [--keys K] [--reps R] [--no-baseline]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from theia_amd import TadEngine  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--values", default="1000000,10000000")
ap.add_argument("--shares", default="0.001,0.1,0.5,0.99")
ap.add_argument("--keys", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=17)
ap.add_argument("--no-baseline", action="store_true")
args = ap.parse_args()

WIDTH = 30
COPIES = 20      # device-to-device copies per timed burst of (c)


def names(n):
    """n distinct 30-byte names in Arrow's layout, built without a Python loop"""
    rows = np.empty((n, WIDTH), dtype=np.uint8)
    rows[:, :11] = np.frombuffer(b"deployment-", dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    for k in range(10):
        rows[:, 20 - k] = 48 + (i // 10 ** k) % 10
    rows[:, 21:] = np.frombuffer(b"-abcdefgh", dtype=np.uint8)
    return np.arange(n + 1, dtype=np.int64) * WIDTH, rows.reshape(-1)


def device_bytes(eng, a):
    base = DeviceArray.from_host(eng, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8), dtype=np.uint64))
    return base.view(0, a.size, np.uint8)


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def restore(eng, vocab, keys):
    sd = eng.string_dict(1, 1)
    sd.load(vocab)
    kd = eng.key_dict(2, 1)
    kd.load(*keys)
    return sd, kd


def select(vocab, keys, survive):
    """the host's selection: the values some key uses or the mask names, renumbered densely; the keys' column 0 through the renumbering"""
    off, data = vocab
    cols, side = keys
    used = survive.copy()
    used[cols[0]] = True
    remap = np.where(used, np.cumsum(used) - 1, -1)
    lens = np.diff(off)
    noff = np.zeros(int(used.sum()) + 1, dtype=np.int64)
    np.cumsum(lens[used], out=noff[1:])
    return (noff, data[np.repeat(used, lens)]), ([remap[cols[0]], cols[1]], side)


def one_shape(eng, n, share):
    rng = np.random.default_rng(args.seed)
    vocab = names(n)
    m = max(int(round(n * share)), 1)
    alive = np.sort(rng.choice(n, m, replace=False))
    survive = np.zeros(n, dtype=bool)
    survive[alive] = True
    keys = ([alive[rng.integers(0, m, args.keys)].astype(np.int64), np.arange(args.keys, dtype=np.int64)], np.zeros(args.keys, np.uint8))
    want_vocab, want_keys = select(vocab, keys, survive)
    res = {"bench": "strdict_retire", "values": n, "share": share, "survivors": m, "keys": args.keys, "bytes_per_name": WIDTH}
    a_ms, b_ms, dev_ms, parts = [], [], [], {"mark": [], "compact": [], "recode": []}
    for rep in range(args.reps):
        # (a)
        sd, kd = restore(eng, vocab, keys)
        mask = device_bytes(eng, survive.astype(np.uint8))
        t0 = time.perf_counter()
        used, _ = kd.used_codes(0, n, into=mask)
        t1 = time.perf_counter()
        remap, st = sd.compact(used, out="device")
        t2 = time.perf_counter()
        kd.recode({0: remap})
        t3 = time.perf_counter()
        a_ms.append((t3 - t0) * 1e3)
        dev_ms.append(st["ms_total"])
        for name, dt in zip(("mark", "compact", "recode"), (t1 - t0, t2 - t1, t3 - t2)):
            parts[name].append(dt * 1e3)
        if rep == 0:
            got_off, got_data = sd.export()
            got_cols, got_side = kd.export()
            res["identical"] = bool(np.array_equal(got_off, want_vocab[0]) and np.array_equal(got_data, want_vocab[1]) and
                                    all(np.array_equal(g, w) for g, w in zip(got_cols, want_keys[0])) and np.array_equal(got_side, want_keys[1]))
            res["compact_stats"] = st
            if not res["identical"]:
                raise SystemExit("strdict_retire_bench: the compacted dictionaries differ from the selection of their exports")
            # (c) a device-to-device copy of as many bytes as the arena copy moves
            total = int(st["arena_used_after"])
            src, dst, word = DeviceArray(eng, total // 8 + 1, np.uint64), DeviceArray(eng, total // 8 + 1, np.uint64), np.zeros(1, np.uint64)
            def burst(n_copies):      # n device-to-device copies behind each other; reading one word back ends them (the copies are asynchronous)
                tc = time.perf_counter()
                for _ in range(n_copies):
                    eng._check(eng._lib.tad_copy_to_device(eng._h, dst.ptr, src.ptr, total))
                eng._check(eng._lib.tad_copy_to_host(eng._h, word.ctypes.data, dst.ptr, 8))
                return (time.perf_counter() - tc) * 1e3
            burst(COPIES)
            # the read-back alone is the floor of this clock; it is taken off and the rest divided by the copies
            floor = float(np.median([burst(0) for _ in range(9)]))
            c_ms = [(burst(COPIES) - floor) / COPIES for _ in range(max(args.reps, 5))]
            res["c_copy_floor_ms"] = floor
            res["c_copy_of_the_survivors_bytes_ms"] = summary(c_ms)
            src.free(), dst.free()
        remap.free()
        sd.close(), kd.close()
        if args.no_baseline:
            continue
        # (b)
        sd, kd = restore(eng, vocab, keys)
        t0 = time.perf_counter()
        nv, nk = select(sd.export(), kd.export(), survive)
        fsd, fkd = eng.string_dict(2 * m, 2 * int(nv[1].size)), eng.key_dict(2, 2 * args.keys)
        fsd.load(nv)
        fkd.load(*nk)
        b_ms.append((time.perf_counter() - t0) * 1e3)
        for x in (sd, kd, fsd, fkd):
            x.close()
        print("# %d values, share %g, rep %d: chain %.3f ms, export / select / import %.3f ms" % (n, share, rep + 1, a_ms[-1], b_ms[-1]), file=sys.stderr, flush=True)
    res["a_chain_ms"] = summary(a_ms)
    res["a_parts_ms"] = {k: summary(v) for k, v in parts.items()}
    res["a_compact_device_ms"] = summary(dev_ms)
    res["c_compact_call_over_copy"] = res["a_compact_device_ms"]["median"] / max(res["c_copy_of_the_survivors_bytes_ms"]["median"], 1e-9)
    if b_ms:
        res["b_export_select_import_ms"] = summary(b_ms)
        res["a_below_b_ranges_apart"] = bool(max(a_ms) < min(b_ms))
    print(json.dumps(res), flush=True)


def main():
    eng = TadEngine(device=0)
    for n in [int(float(x)) for x in args.values.split(",")]:
        for share in [float(x) for x in args.shares.split(",")]:
            one_shape(eng, n, share)
    eng.close()


if __name__ == "__main__":
    main()
