#!/usr/bin/env python3
"""Timing of retiring dead keys (tad_state_compact + tad_keydict_compact) against the only remedy a host had before: export everything,
select on the CPU, import into a fresh state and a fresh dictionary.

Shape: the second-resolution `max` shape of tools/stream_trim_bench.py (conn) with CHURN.  Every hour --cohort new connections appear
(two-column tuples through a key dictionary, ids in order of first appearance) and live for --life hours; an hourly batch of --rows / 24
rows is spread over the connections alive in it.  The state (TAD_STATE_HISTORY | SERIES | TIMES) is trimmed to the newest --window hours
before every batch once the window is full, so after --hours hours most keys it ever saw are unseen.
Then, one engine, the same data for both sides (restored from one host snapshot before every repetition, not timed):
  (a) tad_state_compact(0) + tad_keydict_compact;
  (b) every export -> numpy selection of the keys with n > 0 -> a fresh state and a fresh dictionary with every import;
after a bit-identity check of (a)'s exports against (b)'s selection; alternating, --reps each, median (min-max), wall clock.
  (c) the next EWMA tad_run_stream batches (five minutes each, through each side's own dictionary) and tad_state_bytes +
      tad_keydict_bytes on the compacted state and on an uncompacted copy, alternating, --reps each.
Prints one JSON line.  profiles/key_retire_kernel_stats.csv: `rocprofv3 --kernel-trace --stats -- python tools/key_retire_bench.py --reps 1
--no-baseline --retire-idle`, the dispatches of tad_compact.hip (--retire-idle compacts with retire_before_t = the window's start on an
untrimmed copy, so that k_compact_copy moves the survivors' segments; the unseen-only compaction of (a) moves nothing).
usage: python tools/key_retire_bench.py [--rows N] [--hours H] [--window W] [--cohort C] [--life L] [--reps R] [--no-baseline] [--retire-idle]"""
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
ap.add_argument("--rows", type=int, default=100_000_000, help="rows per day")
ap.add_argument("--hours", type=int, default=24)
ap.add_argument("--window", type=int, default=6)
ap.add_argument("--cohort", type=int, default=250_000, help="new connections per hour")
ap.add_argument("--life", type=int, default=4, help="hours a connection lives")
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--seed", type=int, default=13)
ap.add_argument("--no-baseline", action="store_true")
ap.add_argument("--retire-idle", action="store_true")
args = ap.parse_args()

T0 = 1660202814
HOUR = 3600
SKIP = np.uint64((1 << 64) - 1)
STATE_FIELDS = ("n", "avg", "m2", "ewma", "last_t")


def rows_of(h, lo_s=0, hi_s=HOUR):
    """the rows of seconds [lo_s, hi_s) of hour h (host): connection, time, value"""
    rng = np.random.default_rng(args.seed * 100_000 + h * 64 + lo_s // 300)
    n = args.rows // 24 * (hi_s - lo_s) // HOUR
    first = max(0, h - args.life + 1) * args.cohort                       # the cohorts of hours h - life + 1 .. h are alive
    conn = rng.integers(first, (h + 1) * args.cohort, size=n, dtype=np.int64)
    t = T0 + h * HOUR + rng.integers(lo_s, hi_s, size=n).astype(np.int64)
    v = (1_000_000 + (conn.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 30) + rng.integers(0, 1 << 20, size=n).astype(np.uint64))
    return conn, t, v


def tuple_cols(conn):
    return [conn, (conn % 50_000) + 1024]                                  # (connection, a port): the connection alone is distinct


def feed(eng, st, d, conn, t, v):
    cols = [DeviceArray.from_host(eng, c) for c in tuple_cols(conn)]
    ids, _, fr, _ = d.encode(cols, max_new=0)
    if d.num_keys() > st.num_keys:
        st.resize(d.num_keys())
    dt, dv = DeviceArray.from_host(eng, t), DeviceArray.from_host(eng, v)
    t0 = time.perf_counter()
    r = eng.run_stream(st, ids, dt, dv, value_op="max")
    wall = (time.perf_counter() - t0) * 1e3
    ms = r.stats["ms_total"]
    r.close()
    for x in cols + [ids, fr, dt, dv]:
        x.free()
    return ms, wall


def snapshot(st, d):
    return {"state": st.export(), "history": st.export_history(), "series": st.export_series(), "times": st.export_times(), "dict": d.export()}


def restore(eng, snap):
    K = snap["state"]["n"].size
    st = eng.state_create(K, history=True, series=True, times=True)
    st.load(snap["state"])
    st.load_series(*snap["series"])
    st.load_times(snap["times"])
    st.load_history(*snap["history"])
    d = eng.key_dict(2, 1)
    d.load(*snap["dict"])
    return st, d


def select(snap, live):
    per_point = np.repeat(live, snap["series"][0].astype(np.int64))
    return {"state": {f: snap["state"][f][live] for f in STATE_FIELDS}, "history": (snap["history"][0][live], snap["history"][1][per_point]),
            "series": (snap["series"][0][live], snap["series"][1][per_point]), "times": snap["times"][per_point],
            "dict": ([c[live] for c in snap["dict"][0]], snap["dict"][1][live])}


def same(a, b):
    ok = all(np.array_equal(np.ascontiguousarray(a["state"][f]).view(np.uint8), np.ascontiguousarray(b["state"][f]).view(np.uint8)) for f in STATE_FIELDS)
    ok = ok and all(np.array_equal(a[p][i], b[p][i]) for p in ("history", "series") for i in (0, 1)) and np.array_equal(a["times"], b["times"])
    return bool(ok and all(np.array_equal(x, y) for x, y in zip(a["dict"][0], b["dict"][0])) and np.array_equal(a["dict"][1], b["dict"][1]))


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def main():
    eng = TadEngine(device=0)
    st = eng.state_create(1, history=True, series=True, times=True)
    d = eng.key_dict(2, 1)
    idle_twin = None
    for h in range(args.hours):
        if h >= args.window:
            st.trim(keep_from=T0 + (h - args.window) * HOUR)
        ms, _ = feed(eng, st, d, *rows_of(h))
        print("# hour %d: %d keys, %d points, stream %.3f ms" % (h + 1, st.num_keys, st.series_points(), ms), file=sys.stderr, flush=True)
    keep_from = T0 + (args.hours - args.window) * HOUR
    res = {"bench": "key_retire", "rows_per_day": args.rows, "hours": args.hours, "window_h": args.window, "cohort": args.cohort, "life_h": args.life}
    if args.retire_idle:      # for the kernel trace: an untrimmed copy of the window's keys, compacted by time — the survivors' segments move
        snap = snapshot(st, d)
        idle_twin, dt = restore(eng, snap)
        extra = rows_of(args.hours, 0, 300)
        feed(eng, idle_twin, dt, *extra)
        remap, cs = idle_twin.compact(T0 + args.hours * HOUR)
        dt.compact(remap)
        res["retire_idle"] = cs
        idle_twin.close(), dt.close()
    st.trim(keep_from=keep_from)
    snap = snapshot(st, d)
    live = snap["state"]["n"] > 0
    K, m = int(live.size), int(live.sum())
    res.update({"keys_before": K, "keys_after": m, "series_points": int(snap["times"].size)})
    print("# %d keys, %d alive, %d series points" % (K, m, snap["times"].size), file=sys.stderr, flush=True)
    st.close(), d.close()
    want = select(snap, live)
    a_ms, b_ms, a_dev_ms = [], [], []
    for rep in range(args.reps):
        # (a)
        sa, da = restore(eng, snap)
        t0 = time.perf_counter()
        remap, cs = sa.compact(0, out="device")
        da.compact(remap)
        a_ms.append((time.perf_counter() - t0) * 1e3)
        a_dev_ms.append(cs["ms_total"])
        if rep == 0:
            res["identical"] = same(snapshot(sa, da), want) and cs["keys_after"] == m and cs["series_points_moved"] == 0
            res["compact_stats"] = cs
            res["bytes_compacted"] = sa.nbytes() + da.nbytes()
            if not res["identical"]:
                raise SystemExit("key_retire_bench: the compacted state differs from the selection of its exports")
        remap.free()
        sa.close(), da.close()
        if args.no_baseline:
            continue
        # (b)
        sb, db = restore(eng, snap)
        t0 = time.perf_counter()
        got = select(snapshot(sb, db), sb.export()["n"] > 0)
        fresh = eng.state_create(max(m, 1), history=True, series=True, times=True)
        fresh.load(got["state"])
        fresh.load_series(*got["series"])
        fresh.load_times(got["times"])
        fresh.load_history(*got["history"])
        fd = eng.key_dict(2, 2 * m)
        fd.load(*got["dict"])
        b_ms.append((time.perf_counter() - t0) * 1e3)
        for x in (sb, db, fresh, fd):
            x.close()
        print("# rep %d: compact %.3f ms, export / select / import %.3f ms" % (rep + 1, a_ms[-1], b_ms[-1]), file=sys.stderr, flush=True)
    res["a_compact_ms"] = summary(a_ms)
    res["a_state_compact_device_ms"] = summary(a_dev_ms)
    if b_ms:
        res["b_export_select_import_ms"] = summary(b_ms)
        res["bar_a_below_b_ranges_apart"] = bool(res["a_compact_ms"]["median"] < res["b_export_select_import_ms"]["median"] and max(a_ms) < min(b_ms))
    # (c) the next batches on the compacted state and on an uncompacted copy
    sc, dc = restore(eng, snap)
    remap, _ = sc.compact(0)
    dc.compact(remap)
    su, du = restore(eng, snap)
    c = {"compacted_ms": [], "uncompacted_ms": [], "compacted_wall_ms": [], "uncompacted_wall_ms": []}
    for i in range(args.reps):
        batch = rows_of(args.hours, 300 * i, 300 * (i + 1))
        for name, s_, d_ in (("compacted", sc, dc), ("uncompacted", su, du)) if i % 2 == 0 else (("uncompacted", su, du), ("compacted", sc, dc)):
            ms, wall = feed(eng, s_, d_, *batch)
            c[name + "_ms"].append(ms)
            c[name + "_wall_ms"].append(wall)
    res["c_next_batch"] = {k: summary(v) for k, v in c.items()}
    res["c_bytes"] = {"compacted": sc.nbytes() + dc.nbytes(), "uncompacted": su.nbytes() + du.nbytes(), "compacted_keys": sc.num_keys, "uncompacted_keys": su.num_keys}
    for x in (sc, dc, su, du):
        x.close()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
