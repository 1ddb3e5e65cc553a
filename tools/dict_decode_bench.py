"""tad_strdict_decode against what it replaces and against a plain copy ("Decoding on the device").

One MI355X, one engine per library, the variants in alternating order; median and range of `--reps` calls after a warm-up, every call
ending in a host synchronisation.
  (a) tad_strdict_decode, device codes -> device strings: `--rows` codes drawn uniformly and in a result-like pattern (runs of about 10
      equal codes) from vocabularies of `--distinct` pod-name-like strings — with the shipped library (the tiled copy) and, when
      `--rows-library` names a build made with -DTAD_SD_DECODE_ROWS (python tools/build_variants.py rows:TAD_SD_DECODE_ROWS), with the
      lane-per-row copy, on a second engine of the same process;
  (b) what (a) replaces: StringDict.values() — the whole vocabulary to the host — and a take of the same codes there (pyarrow's);
  (c) the yardstick: a device-to-device tad_copy_to_device of as many bytes as the decode writes; the decode is reported as a fraction
      of its rate;
  (d) StreamingAnomalyDetection.job (EWMA, svc mode, no filter) at `--job-keys` keys — `--tree PATH` runs this part alone on another
      checkout of the project (the parent commit, built there), so that both job times come from the same box and the same script.
Writes profiles/dict_decode_bench.json (or --out).  No threshold: the numbers go into DESIGN.md §5 with their ranges.

    python tools/dict_decode_bench.py [--rows 1000000,10000000] [--distinct 1000,100000,10000000] [--reps 20] [--rows-library PATH]
    python tools/dict_decode_bench.py --job-only --tree /path/to/parent/checkout --out profiles/dict_decode_bench_parent.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "calls": reps}


def pod_names(distinct):
    """`distinct` names like "coredns-5d78c9869d-0000123" in Arrow's layout: (offsets int64, data uint8)"""
    i = np.arange(distinct, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(24)
    prefix = np.array(["coredns", "antrea-agent", "kube-proxy", "theia-manager"])[(i % np.uint64(4)).astype(np.int64)]
    names = np.char.add(np.char.add(prefix, "-"), np.char.add(np.char.mod("%010x", h.astype(np.int64)), np.char.mod("-%07d", i.astype(np.int64))))
    raw = np.char.encode(names, "ascii")
    offsets = np.zeros(distinct + 1, dtype=np.int64)
    np.cumsum(np.char.str_len(raw), out=offsets[1:])
    return offsets, np.frombuffer(b"".join(raw.tolist()), dtype=np.uint8)


def code_patterns(distinct, rows, rng):
    runs = rng.integers(0, distinct, rows // 10 + 1)
    return {"uniform": rng.integers(0, distinct, rows).astype(np.int64), "result_like": np.repeat(runs, 10)[:rows].astype(np.int64)}


def decode_part(args, out):
    import ctypes as C
    from theia_amd import TadEngine, _capi as capi
    from theia_amd.engine import DeviceArray
    engines = {"tiled": TadEngine(device=0)}
    if args.rows_library:
        engines["lane_per_row"] = TadEngine(device=0, library_path=args.rows_library)
    rng = np.random.default_rng(1)
    for distinct in [int(x) for x in args.distinct.split(",")]:
        vocab = pod_names(distinct)
        dicts = {}
        for name, eng in engines.items():
            dicts[name] = eng.string_dict(distinct, int(vocab[0][-1]))
            dicts[name].load(vocab)
        for rows in [int(x) for x in args.rows.split(",")]:
            for pattern, codes in code_patterns(distinct, rows, rng).items():
                res = {"distinct": distinct, "rows": rows, "pattern": pattern}
                total = int((vocab[0][1:] - vocab[0][:-1])[codes].sum())
                res["bytes"] = total
                # every library's call on its own engine, into buffers allocated once: the C call alone, which ends in its own synchronisation
                calls = {}
                keep = []
                for name, eng in engines.items():
                    dc, do, dd = DeviceArray.from_host(eng, codes), DeviceArray(eng, rows + 1, np.int64), DeviceArray(eng, total // 8 + 1, np.uint64)
                    keep += [dc, do, dd]
                    need = C.c_uint64()

                    def call(eng=eng, d=dicts[name], dc=dc, do=do, dd=dd, need=need):
                        eng._check(eng._lib.tad_strdict_decode(eng._h, d._h, dc.ptr, rows, capi.TAD_MEM_DEVICE, do.ptr, dd.ptr, total, capi.TAD_MEM_DEVICE, C.byref(need)))
                    calls[name] = call
                eng = engines["tiled"]
                src, dst, word = DeviceArray(eng, total // 8 + 1, np.uint64), DeviceArray(eng, total // 8 + 1, np.uint64), np.zeros(1, np.uint64)
                keep += [src, dst]

                def copy():      # the copy is asynchronous for a device source: reading one word back ends it
                    eng._check(eng._lib.tad_copy_to_device(eng._h, dst.ptr, src.ptr, total))
                    eng._check(eng._lib.tad_copy_to_host(eng._h, word.ctypes.data, dst.ptr, 8))
                for _ in range(2):      # alternating order: the second round's numbers are kept
                    for name in engines:
                        res["a_decode_" + name] = timed(calls[name], args.reps)
                    res["c_copy"] = timed(copy, args.reps)
                res["a_tiled_fraction_of_copy_rate"] = res["c_copy"]["median_ms"] / res["a_decode_tiled"]["median_ms"]
                if rows <= args.host_rows:
                    import pyarrow as pa
                    take = pa.array(codes)
                    res["b_values_and_take"] = timed(lambda: dicts["tiled"].values().take(take), max(args.reps // 4, 3), warm=1)
                for d in keep:
                    d.free()
                out["decode"].append(res)
                print(json.dumps(res), flush=True)
        for d in dicts.values():
            d.close()
    for eng in engines.values():
        eng.close()


def job_part(args, out):
    from theia_amd import TadEngine
    from theia_amd.stream_detection import StreamingAnomalyDetection
    rng = np.random.default_rng(2)
    with TadEngine(device=0) as eng:
        for keys in [int(x) for x in args.job_keys.split(",")]:
            names = np.char.add("ns/svc-", np.char.mod("%07d", np.arange(keys)))
            s = StreamingAnomalyDetection(eng, "svc")
            feed_s = 0.0
            for step in range(12):          # twelve points a key, one of them far out: about one result row a key
                value = rng.integers(1_000_000_000, 1_100_000_000, keys).astype(np.uint64)
                if step == 9:
                    value *= np.uint64(30)
                order = rng.permutation(keys)
                flows = {"destinationServicePortName": names[order],
                         "flowEndSeconds": np.full(keys, 1660202800 + 60 * step, dtype=np.int64), "throughput": value[order]}
                t = time.perf_counter()
                s.feed(flows)
                feed_s += time.perf_counter() - t
            rows = []

            def job():
                rows[:] = [s.job("EWMA", "bench")[1]]
            res = {"keys": keys, "feed_s": feed_s, "job": timed(job, max(args.reps // 4, 3), warm=1), "result_rows": 0}
            res["result_rows"] = len(rows[0])
            s.close()
            out["job"].append(res)
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--distinct", default="1000,100000,10000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rows", type=int, default=10_000_000, help="(b) runs for code counts up to this")
    ap.add_argument("--rows-library", default="", help="a build with -DTAD_SD_DECODE_ROWS: the lane-per-row copy, timed beside the shipped one")
    ap.add_argument("--job-keys", default="100000,1000000")
    ap.add_argument("--job-only", action="store_true")
    ap.add_argument("--no-job", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose theia_amd is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_decode_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    out = {"tree": "this commit" if os.path.abspath(args.tree) == ROOT else "another checkout", "cores": os.cpu_count(), "decode": [], "job": []}
    if not args.job_only:
        decode_part(args, out)
    if not args.no_job:
        job_part(args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
