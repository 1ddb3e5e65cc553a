"""GPU: the dense Stage 0 (tad_stage0_part.hip) at every chunk, queue, tile and record edge, bit for bit against the CPU oracle
(DESIGN.md §4 has the table):
  A  pass A and the row chunking: chunk = even(ceil(n / 256)), empty workgroups, the odd last row, the unrolled loop and its tail,
     the sampled layout on tables so small that every count is exact, the region that sends a sorted table to the exact histogram
  B  the plan: bins and key blocks, every widening rule of part_plan_tiles, the record's cell and value fields, the T < 2^16 rule,
     the three lattice modes, part_plan_wc's unforced rules
  C  pass B: the tiles of k_partition_wc and k_partition, the queue fill levels, the 288 parked spills, the wavefront aggregation
  D  pass C: the slice split, the wavefront chunks of the exact walk, the bucket rounds, settle mode, the overflow list exactly full

References: orc.stage0 (a numpy group-by) for engine.aggregate, orc.run_job through check_job of tests/test_gpu_parity.py for the rows
of engine.run with and without emit_all.  No tolerances anywhere.

Every case forces the dense partition path on a small table (stage0="v2", sparse="never": G is always 256 workgroups) and asserts
from host-side numbers that it sits on the edge it is named for BEFORE the engine is asked: the plan from the few lines of Python
below (part_plan_bins, part_plan_tiles, part_plan_wc, part_plan_settle, make_lattice's mode, slice_len_of), the row -> workgroup,
tile and lane mapping from the row index.  Afterwards what the engine exposes: stage0_path, stage0_attempts, hist_sampled,
n_buckets, step, rows_used, n_points.  A constant that changes in the source makes the mirror's literal expectations fail: no case
silently tests the middle of a range.

What cannot be seen from outside and is therefore never relied on: the order in which LDS atomics land (a record's rank inside its
tile, which record is "the last" of a workgroup of more than one thread), the exact record-slot count of a region under the
write-combining pass (fillers), the adaptive queue depths when a workgroup's histogram row is skewed.  Left out: cell_bits 18 .. 24
(grids of >= 2e8 cells), more than 2^32 slots.

Two findings of the mirror, recorded and asserted, not changed: at exactly 986 partitions part_plan_tiles keeps the key block (its
line_parts = kLdsBudget / 162 = 986) while part_plan_wc computes 17 slots and takes 64-byte sectors; and part_plan_wc's unforced
`>= 24 records per run` rule is unreachable (64-byte sectors need >= 987 partitions, where a tile brings at most 10 records each).
The sort-by-tile pass reads tiles of 10240 rows one-sided, 4096 two-sided (part_plan_tiles gives rpt 4 there) and 4096 when generic.

103 cases, 23 s on an MI355X (the slowest: the 262272 x 100 settle cases, 2.4 s each).  That the cases can fail was checked with builds of the
library that compute wrong values inside every buffer, on the host emulator only (DESIGN.md §4 lists them, and the three that no case can see).

The builders are plain functions of seeded numpy, usable without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import tad_oracle as orc
from job_helpers import check_job, lattice

pytestmark = pytest.mark.gpu

# the constants of the kernels and plans, mirrored (a change there must be followed here)
G = 256                        # tad_stage0_part.hip:1490  pl->G: workgroups of pass A and pass B
THREADS = 1024                 # tad_stage0_part.hip:43    kPartThreads
MIN_CELL_BITS, MAX_CELL_BITS = 15, 24    # tad_stage0_part.hip:53
TILE_CELLS = 17744             # tad_stage0_part.hip:54    kTileCells
MAX_PARTS = 2048               # tad_stage0_part.hip:55    kMaxParts
LDS_BUDGET = 156 * 1024        # tad_stage0_part.hip:56    kLdsBudget
WAVE_AGG_MIN = 8               # tad_stage0_part.hip:134   kWaveAggMin
WC_FIXED = 18                  # tad_stage0_part.hip:139   kWcFixedBytes
SAMPLE_MASK = 15               # tad_stage0_part.hip:200   kSampleMask
REGION_UR = 12                 # tad_stage0_part.hip:203   records per lane and batch of the sampled region walk
META_U = 4                     # tad_stage0_part.hip:241   row pairs per thread and iteration of k_meta_hist
CAP_SIGMAS, CAP_INTERVALS = 5.5, 12.0    # tad_stage0_part.hip:358   sampled_capacity
BIG_REGION = 8192              # tad_stage0_part.hip:367   kBigSampledRegion
SPILL_SLOTS = 288              # tad_stage0_part.hip:859   kSpillSlots
SLICE_RECORDS = 1 << 17        # tad_stage0_part.hip:1135  kSliceRecords
WALK_U = 8                     # tad_stage0_part.hip:1231  records per lane and chunk of the exact walk
LINE_PARTS = LDS_BUDGET // (8 * 18 + 18)    # tad_stage0_part.hip:1515  986
SECTOR_PARTS = LDS_BUDGET // (8 * 9 + 18)   # tad_stage0_part.hip:1530  1774
SORT_RPT = (10, 8, 4, 2)       # tad_stage0_part.hip:1552  rows per thread of k_partition
MAX_BINS = 16384               # tad_internal.h:560        kMaxBins
OVERFLOW_CAP = 1 << 20         # tad_engine.h:215          kOverflowCap
NARROW_LIMIT = (1 << 32) - 2   # tad_stage0_part.hip:1735

T0 = 1660202814
U64 = np.uint64
SKIP = orc.KEY_SKIP
DENSE = dict(stage0="v2", sparse="never")
PASSES = ("sort", "wc", "wc_sectors")
PP = {"auto": 0, "sort": 1, "wc": 2, "wc_sectors": 3}
assert (LINE_PARTS, SECTOR_PARTS) == (986, 1774)


# ------------------------------------------------------------------ the mirror
def ceil_div(a, b):
    return -(-a // b)


def plan_bins(n, K):
    """part_plan_bins (tad_stage0_part.hip:1484)"""
    sb = 0
    while ceil_div(K, 1 << sb) > MAX_BINS:
        sb += 1
    chunk = (ceil_div(n, G) + 1) & ~1
    return SimpleNamespace(shift_bin=sb, nbins=ceil_div(K, 1 << sb), chunk=chunk)


def plan_tiles(K, T, has2=False, shift_bin=None):
    """part_plan_bins' shift_bin + part_plan_tiles (tad_stage0_part.hip:1497); None = no tile plan (direct scatter)"""
    sb = plan_bins(1, K).shift_bin if shift_bin is None else shift_bin
    if T == 0 or T >= 1 << 16:
        return None
    parts = lambda c: ceil_div(K, 1 << c)
    rounds = lambda c: ceil_div(T, TILE_CELLS >> c) if TILE_CELLS >> c else 1 << 30
    fit = max([c for c in range(14) if (T << c) <= TILE_CELLS], default=-1)
    sp = max(fit, sb)
    while parts(sp) > MAX_PARTS and sp < 13:
        sp += 1
    if parts(sp) > MAX_PARTS:
        return None
    while sp > sb and (1 << (sp - 1)) >= K:
        sp -= 1
    if parts(sp) > LINE_PARTS:
        c = sp
        while c < 13 and parts(c) > LINE_PARTS:
            c += 1
        if parts(c) <= LINE_PARTS and (1 << c) <= TILE_CELLS and rounds(c) <= 2 * rounds(sp) and rounds(c) <= 4:
            sp = c
    if parts(sp) > SECTOR_PARTS and sp < 13 and parts(sp + 1) <= SECTOR_PARTS and (1 << (sp + 1)) <= TILE_CELLS and rounds(sp + 1) <= 8:
        sp += 1
    if (1 << sp) > TILE_CELLS:
        return None
    KP = 1 << sp
    cells_all = KP * T
    cb = MIN_CELL_BITS
    while cb < MAX_CELL_BITS and (1 << cb) - 1 <= cells_all:
        cb += 1
    if (1 << cb) - 1 <= cells_all:
        return None
    tb = min(TILE_CELLS >> sp, T)
    n_chunks = ceil_div(T, tb)
    tb = ceil_div(T, n_chunks)
    nparts = parts(sp)
    fixed = (nparts + 4) * 16 + 64
    rpt = next((r for r in SORT_RPT if r * THREADS * (2 if has2 else 1) * 10 + fixed <= LDS_BUDGET), 0)
    if rpt == 0:
        return None
    return SimpleNamespace(shift_bin=sb, shift_part=sp, KP=KP, nparts=nparts, bins_per_part=1 << (sp - sb), cell_bits=cb, tb=tb,
                           n_chunks=n_chunks, rpt=rpt, value_limit=1 << (64 - cb))


def plan_wc(pl, slots, has2=False, partition_pass="auto"):
    """part_plan_wc (tad_stage0_part.hip:1623) -> (wc_cap, wc_sec, wc_rpt), or None when the sort-by-tile pass runs"""
    pp, mult = PP[partition_pass], 2 if has2 else 1
    if pp == 1:
        return None
    per = (LDS_BUDGET - 16) // pl.nparts
    if per < WC_FIXED + 8 * 9:
        return None
    cap = min((per - WC_FIXED) // 8, 64)
    sec = 16 if cap >= 18 and pp != 3 else 8
    if sec == 8:
        cap = min(cap, 16)
    forced = pp >= 2
    if not forced and sec == 8 and pl.rpt * THREADS * mult // pl.nparts >= 24:
        return None
    if not forced and 2.0 * THREADS * mult / pl.nparts > cap - (sec - 1):
        return None
    lam4 = 4.0 * THREADS * mult / pl.nparts
    rpt = 4 if not has2 and cap - (sec - 1) >= 2.0 * lam4 + 4.0 else 2
    if slots + (sec - 1) * G * pl.nparts >= 1 << 32:
        return None
    return SimpleNamespace(cap=cap, sec=sec, rpt=rpt)


def plan_settle(pl, T, narrow):
    """part_plan_settle (tad_stage0_part.hip:1592) -> (kt, rounds), or None when refused"""
    kt = min((LDS_BUDGET - 64) // (T * (4 if narrow else 9) + 9), pl.KP, 1024)
    if kt < 8:
        return None
    rounds = ceil_div(pl.KP, kt)
    if rounds > pl.n_chunks + 1 and rounds > 1:
        return None
    return ceil_div(pl.KP, rounds), rounds


def lattice_mode(step, nb):
    """make_lattice (tad_rows.h)"""
    if step == 1:
        return 0
    return 1 if step < (1 << 32) and (nb == 0 or nb - 1 <= ((1 << 32) - 1) // step) else 2


def slice_len_of(sampled, slots, nparts):
    """slice_len_of (tad_stage0_part.hip:1703)"""
    mean = slots // nparts
    return max(mean + mean // 2, 3 * SLICE_RECORDS if sampled else SLICE_RECORDS)


def sampled_capacity(est):
    """sampled_capacity (tad_stage0_part.hip:359), rounded to 16 records (launch_part_offsets: round_mask 15)"""
    c = int(est + CAP_SIGMAS * np.sqrt(est * (SAMPLE_MASK + 1.0)) + CAP_INTERVALS * (SAMPLE_MASK + 1.0))
    return (c + 15) & ~15


def sort_tile_rows(pl, has2, generic):
    """rows per tile of k_partition as launch_partition picks it (tad_stage0_part.hip:1767-1790)"""
    rpt = min(pl.rpt, 4) if generic else pl.rpt
    if not generic:
        rpt = {10: 8 if has2 else 10, 8: 8, 6: 4, 4: 4}.get(rpt, 2)
    else:
        rpt = 4 if rpt >= 4 else 2
    return rpt * THREADS


def expected_path(pl, slots, has2, partition_pass):
    return 3 if plan_wc(pl, slots, has2, partition_pass) is not None else 2


# ------------------------------------------------------------------ shared helpers
def agg_check(engine, k, t, v, K, agg, paths, k2=None, want=None, **kw):
    """engine.aggregate against the numpy group-by"""
    okw = {a: kw[a] for a in ("end_time",) if a in kw}
    pk, pt, pv = want if want is not None else orc.stage0(k, t, v, "sum" if agg else "max", k2, **okw)
    pts = engine.aggregate(k, t, v, K, agg_flow=agg, key_id2=k2, **kw)
    assert pts.stats["stage0_path"] in paths, pts.stats["stage0_path"]
    assert pts.n_points == pk.size == pts.stats["n_points"]
    assert (pts["key_id"] == pk).all() and (pts["flow_end_s"] == pt).all() and (pts["value"] == pv).all()
    return pts


def job_check(engine, algo, k, t, v, K, agg, want=None, **kw):
    """check_job of tests/test_gpu_parity.py; with `want` (an orc.run_job result shared between plans) the same assertions without the
    oracle's second run"""
    if want is None:
        return check_job(engine, algo, k, t, v, K, agg_flow=agg, **kw)
    allp = engine.run(algo, k, t, v, K, agg_flow=agg, emit_all=True, **kw)
    pk, pt, pv = want["points"]
    assert allp.n_rows == want["n_points"] == allp.stats["n_points"] and allp.stats["n_keys"] == want["n_keys"]
    assert (allp["key_id"] == pk).all() and (allp["flow_end_s"] == pt).all() and (allp["throughput"] == orc.u64_to_f64(pv)).all()
    assert (allp["stddev"] == np.repeat(want["sigma"], np.diff(want["ptr"]))).all()
    assert (allp["algo_calc"] == want["calc_all"]).all() and (allp["anomaly"].astype(bool) == want["anomaly_all"]).all()
    assert allp.stats["n_anomalies"] == want["n_anomalies"]
    res = engine.run(algo, k, t, v, K, agg_flow=agg, **kw)
    assert res.n_rows == want["n_anomalies"] == res.stats["n_anomalies"]
    for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
        assert (res[f] == want[f]).all(), f
    return res, want


def dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"), hists=("exact",), aggs=("svc", ""), jobs=(("EWMA", "svc"),), k2=None,
                 attempts=1, share=True, **kw):
    """aggregate and the jobs under every (pass, histogram): bit for bit, on the path the mirror names, in `attempts` attempts, with the
    lattice of the live rows, every live row used"""
    sides = [k] if k2 is None else [k, k2]
    live = np.concatenate([np.broadcast_to(t, s.shape)[s != SKIP] for s in sides])
    if kw.get("end_time"):
        live = live[live < kw["end_time"]]
    t0, step, nb = lattice(live)                      # (a hint is the same lattice, or too short and then replaced by this one)
    slots = k.size * len(sides)
    okw = {a: kw[a] for a in ("end_time",) if a in kw}
    want_agg = {agg: orc.stage0(k, t, v, "sum" if agg else "max", k2, **okw) for agg in aggs}
    want_job = {(algo, agg): orc.run_job(algo, k, t, v, agg_flow=agg, key_id2=k2, **okw) for algo, agg in jobs} if share else {}
    out = None
    for p in passes:
        path = expected_path(pl, slots, k2 is not None, p)
        for h in hists:
            with engine.plan(partition_pass=p, histogram=h, **DENSE):
                for agg in aggs:
                    pts = agg_check(engine, k, t, v, K, agg, (path,), k2, want=want_agg[agg], **kw)
                    assert pts.stats["stage0_attempts"] == attempts and pts.stats["hist_sampled"] == (h == "sampled" and attempts == 1), (p, h)
                for algo, agg in jobs:
                    jkw = dict(kw, key_id2=k2) if k2 is not None else kw
                    res, _ = job_check(engine, algo, k, t, v, K, agg, want=want_job.get((algo, agg)), **jkw)
                    st = res.stats
                    assert (st["stage0_path"], st["stage0_attempts"]) == (path, attempts), (p, h, st["stage0_path"], st["stage0_attempts"])
                    assert st["hist_sampled"] == (h == "sampled" and attempts == 1), (p, h)
                    assert (st["n_buckets"], st["step"], st["rows_used"]) == (nb, step, live.size), (p, h)
                    out = res if out is None else out
    return out


def rows_on(points, seed, vlo=1, vhi=3_000_000_000, step=1, shuffle=True):
    """points: [(key, bucket array, rows per point)] -> key, time, value columns, rows in a seeded arbitrary order"""
    kk, tt = [], []
    for key, b, r in points:
        b = np.asarray(b, dtype=np.int64)
        kk.append(np.repeat(np.full(b.size, key, dtype=U64), r))
        tt.append(np.repeat(b, r))
    k, t = np.concatenate(kk), T0 + step * np.concatenate(tt)
    rng = np.random.default_rng(seed)
    v = rng.integers(vlo, vhi, size=k.size).astype(U64)
    o = rng.permutation(k.size) if shuffle else np.arange(k.size)
    return np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o])


def random_rows(n, K, T, seed, step=1):
    """n rows on keys [0, K) and buckets [0, T): key K - 1, bucket 0 and bucket T - 1 present"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, K, size=n).astype(U64)
    sec = rng.integers(0, T, size=n).astype(np.int64)
    k[0], sec[0], sec[-1] = K - 1, 0, T - 1
    return k, T0 + step * sec, rng.integers(1, 3_000_000_000, size=n).astype(U64)


def wg_rows(n, chunk):
    """rows of every workgroup: [(lo, hi)] of the 256"""
    return [(min(g * chunk, n), min((g + 1) * chunk, n)) for g in range(G)]


# ================================================================== A. pass A and the row chunking
#            n: (chunk, workgroups with rows, rows of the last of them)
A1_EDGES = {1: (2, 1, 1), 2: (2, 1, 2), 3: (2, 2, 1), 255: (2, 128, 1), 256: (2, 128, 2), 257: (2, 129, 1), 511: (2, 256, 1),
            512: (2, 256, 2), 513: (4, 129, 1), 767: (4, 192, 3), 1025: (6, 171, 5)}


@pytest.mark.parametrize("n", sorted(A1_EDGES))
def test_row_counts_at_chunk_and_pair_edges(engine, n):
    """part_plan_bins / k_meta_hist / both pass B kernels: chunk = even(ceil(n / 256)), workgroups whose lo >= n, an odd last row that
    thread 0 reads alone.  The last row carries the table's only maximum time: dropped, n_buckets changes."""
    K, T = 5, 30
    rng = np.random.default_rng(100 + n)
    k = rng.integers(0, K, size=n).astype(U64)
    sec = rng.integers(0, T - 1, size=n).astype(np.int64)
    sec[:2] = (0, 1)[:n]                              # (two rows: the lattice is those two, step 29)
    sec[-1] = T - 1 if n > 1 else 0
    t = T0 + sec
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    k2 = rng.integers(0, K, size=n).astype(U64)
    k2[rng.random(n) < 0.1] = SKIP
    chunk = plan_bins(n, K).chunk
    active = [(lo, hi) for lo, hi in wg_rows(n, chunk) if hi > lo]
    assert (chunk, len(active), active[-1][1] - active[-1][0]) == A1_EDGES[n] and chunk % 2 == 0
    assert int((t == t.max()).sum()) == 1 and t[-1] == t.max() and lattice(t)[1:] == {1: (1, 1), 2: (T - 1, 2)}.get(n, (1, T))
    pl = plan_tiles(K, lattice(t)[2])
    assert (pl.KP, pl.nparts, pl.cell_bits) == (8, 1, 15)
    for two in (None, k2):
        for end in (0, T0 + T):            # te < end_time keeps every row, the last one by one second: the GENERIC kernels
            kw = dict(end_time=end) if end else {}
            dense_checks(engine, k, t, v, K, pl, passes=PASSES, hists=("exact", "sampled"), aggs=("pod" if two is not None else "svc",),
                         jobs=(("EWMA", "pod" if two is not None else "svc"),), k2=two, **kw)


def meta_tail_rows(n, chunk):
    """rows that k_meta_hist reads in its tail loop or as the odd last row (boolean per row): thread tid holds the row pairs
    it * 4096 + u * 1024 + tid while `tid + it * 4096 + 3 * 1024 < npair`"""
    r = np.arange(n, dtype=np.int64)
    g = r // chunk
    lo = g * chunk
    hi = np.minimum(lo + chunk, n)
    npair = (hi - lo) >> 1
    pair = (r - lo) >> 1
    it, tid = pair // (META_U * THREADS), pair % THREADS
    return (it * META_U * THREADS + tid + (META_U - 1) * THREADS >= npair) | (pair >= npair)


@functools.lru_cache(maxsize=None)
def tail_table(n):
    K, T = 3000, 40
    k, t, v = orc.synth_rows(0, n, K - 100, T)
    tail = meta_tail_rows(n, plan_bins(n, K).chunk)
    k = np.where(tail, U64(K - 100) + (np.arange(n, dtype=U64) % U64(100)), k)      # keys of the tail's rows occur nowhere else
    return k, t, v, K, T, tail


@pytest.mark.parametrize("n,chunk,tail_pairs_wg0", [(2_096_640, 8190, [1023, 2047, 3071]), (2_097_152, 8192, []), (2_097_153, 8194, [4096])])
def test_pass_a_unrolled_loop_and_its_tail(engine, n, chunk, tail_pairs_wg0):
    """k_meta_hist: `i + 3 * 1024 < npair` (8192 rows per iteration), then the tail loop: npair 4095 (thread 1023 alone takes the
    tail), 4096 (no tail), 4097 (thread 0 alone).  A tail that is not histogrammed leaves its keys' regions empty."""
    k, t, v, K, T, tail = tail_table(n)
    assert plan_bins(n, K).chunk == chunk and chunk // 2 == {8190: 4095, 8192: 4096, 8194: 4097}[chunk]
    assert np.flatnonzero(tail[:chunk]).tolist() == [r for p in tail_pairs_wg0 for r in (2 * p, 2 * p + 1)]
    if n % 2:
        assert tail[-1] and (n - 255 * chunk) % 2 == 1
    assert not np.isin(k[~tail], k[tail]).any() and (k[tail] >= U64(K - 100)).all()
    pl = plan_tiles(K, T)
    assert lattice(t)[1:] == (60, T) and (pl.KP, pl.nparts) == (256, 12)
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"), aggs=("svc",))


@pytest.mark.parametrize("parts", [1, 16])
@pytest.mark.parametrize("chunk", [766, 768, 770])
def test_sampled_layout_on_small_tables(engine, chunk, parts):
    """k_meta_hist<SAMPLE_H> with fewer than two whole iterations per chunk: every iteration is in the `zone`, the counts are exact but
    the layout is the sampled one (capacity est + 5.5 sqrt(16 est) + 192, slack between fin_lo and fin_hi, pass C's walk of a wavefront
    per region in batches of 12 * 64 records).  One partition: every region holds one batch - 2 / exactly / + 2 records, and every
    wavefront step is on one partition (the downward top-of-region path, [start, fin_lo) empty).  16 partitions: four lanes of every
    wavefront step each, all through the queues."""
    n, T = G * chunk, 30
    K = 5 if parts == 1 else 16 * 512
    pl = plan_tiles(K, T)
    assert plan_bins(n, K).chunk == chunk and (pl.nparts, pl.KP) == ((1, 8) if parts == 1 else (16, 512))
    assert chunk - REGION_UR * 64 in (-2, 0, 2) and chunk < 2 * META_U * THREADS * 2            # one batch of the walk; all `zone`
    rng = np.random.default_rng(chunk + parts)
    r = np.arange(n, dtype=np.int64)
    k = rng.integers(0, K, size=n).astype(U64) if parts == 1 else (((r // 8) % 16) * 512 + rng.integers(0, 512, size=n)).astype(U64)
    lane_part = (k[0:128:2] >> U64(pl.shift_part)).astype(np.int64)                           # wavefront 0, step 0: rows 0, 2, .. 126
    assert np.bincount(lane_part, minlength=parts).tolist() == [64 // parts] * parts and (64 // parts >= WAVE_AGG_MIN) == (parts == 1)
    per_region = np.bincount((r // chunk) * parts + (k >> U64(pl.shift_part)).astype(np.int64), minlength=G * parts)
    assert per_region.sum() == n and (parts != 1 or (per_region == chunk).all())
    assert sampled_capacity(int(per_region.max())) - int(per_region.max()) >= 192
    sec = rng.integers(0, T, size=n).astype(np.int64)
    sec[:2] = (0, T - 1)
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    dense_checks(engine, k, T0 + sec, v, K, pl, passes=PASSES, hists=("sampled",))


def test_big_sampled_region_goes_to_the_exact_histogram():
    """k_part_offsets: a sampled region above 8192 records and above 8 x the partition's mean raises DEV_ERR_REGION_FULL before pass B
    runs: rows sorted by key, chunk 8200, every partition's rows in two chunks.  A fresh engine: the job context remembers."""
    from theia_amd import TadEngine
    K, T, chunk = 128 * 512, 30, 8200
    n = G * chunk
    pl = plan_tiles(K, T)
    assert plan_bins(n, K).chunk == chunk and (pl.KP, pl.nparts, plan_bins(n, K).shift_bin) == (512, 128, 2)
    r = np.arange(n, dtype=np.int64)
    k = ((r // (2 * chunk)) * 512 + r % 512).astype(U64)
    region = sampled_capacity(chunk)
    total = 2 * region + (G - 2) * sampled_capacity(0)
    assert chunk > BIG_REGION and region > BIG_REGION and region * G > 8 * total and (np.diff(k.astype(np.int64) >> 9) >= 0).all()
    rng = np.random.default_rng(5)
    sec = rng.integers(0, T, size=n).astype(np.int64)
    sec[:2] = (0, T - 1)
    t, v = T0 + sec, rng.integers(1, 3_000_000_000, size=n).astype(U64)
    want = orc.run_job("EWMA", k, t, v, agg_flow="svc")
    eng = TadEngine(device=0, plan=dict(partition_pass="wc", histogram="sampled", **DENSE))
    try:
        res = eng.run("EWMA", k, t, v, K, agg_flow="svc")
        assert (res.stats["stage0_attempts"], res.stats["hist_sampled"], res.stats["stage0_path"]) == (2, 0, 3)
        assert res.n_rows == want["n_anomalies"] and res.stats["rows_used"] == n and res.stats["n_points"] == want["n_points"]
        for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
            assert (res[f] == want[f]).all(), f
        agg_check(eng, k, t, v, K, "svc", (3,), want=want["points"])
    finally:
        eng.close()


# ================================================================== B. the plan
#          K: (shift_bin, nbins, KP, nparts, bins_per_part, keys of the last partition)
B1_CASES = {255: (0, 255, 256, 1, 256, 255), 256: (0, 256, 256, 1, 256, 256), 257: (0, 257, 512, 1, 512, 257),
            16384: (0, 16384, 512, 32, 512, 512), 16385: (1, 8193, 512, 33, 256, 1)}


@pytest.mark.parametrize("K", sorted(B1_CASES))
def test_key_counts_at_bin_and_block_edges(engine, K):
    """part_plan_bins / k_part_offsets: bins_per_part bins summed per partition, b1 clamped to nbins, shift_bin > 0 from K = 16385 on.
    The last partition holds KP - 1 keys (K = 255) and one key (K = 16385); key K - 1 and the first key of the last partition carry
    the table's largest sums."""
    T = 30
    pb, pl = plan_bins(7000, K), plan_tiles(K, T)
    last = K - (pl.nparts - 1) * pl.KP
    assert (pb.shift_bin, pb.nbins, pl.KP, pl.nparts, pl.bins_per_part, last) == B1_CASES[K]
    assert pl.nparts * pl.bins_per_part >= pb.nbins and (K != 16385 or pl.nparts * pl.bins_per_part > pb.nbins)      # the clamp
    k, t, v = random_rows(7000, K, T, seed=K)
    top = np.array([K - 1, (pl.nparts - 1) * pl.KP], dtype=U64)
    k = np.concatenate([k, np.repeat(top, 40)])
    t = np.concatenate([t, np.tile(T0 + np.arange(40) % T, 2)])
    v = np.concatenate([v, np.full(80, U64(1 << 44))])
    pk, _, pv = orc.stage0(k, t, v, "sum")
    assert set(pk[pv >= U64(1 << 44)].tolist()) == set(top.tolist())
    dense_checks(engine, k, t, v, K, pl, passes=PASSES, hists=("exact", "sampled"))


#            K, T: (shift_part, nparts, n_chunks, wc_sec under partition_pass="wc")
B2_CASES = {(128 * 985, 100): (7, 985, 1, 16), (128 * 986, 100): (7, 986, 1, 8), (128 * 987, 100): (8, 494, 2, 16),
            (128 * 2048, 100): (8, 1024, 2, 8), (128 * 2049, 100): (9, 513, 3, 16), (1774, 40000): (0, 1774, 3, 8), (1775, 40000): (1, 888, 5, 16)}


@pytest.mark.parametrize("K,T", sorted(B2_CASES))
def test_partition_counts_at_every_widening_rule(engine, K, T):
    """part_plan_tiles: the key block widened at parts > kMaxParts (128 * 2049), at parts > line_parts = 986 if pass C then needs at
    most twice the rounds and no more than 4 (128 * 987; refused at 1774 x 40000: 5 rounds), at parts > sector_parts = 1774 if at most
    8 rounds (128 * 2048; 1775 x 40000).  At exactly 986 partitions the block is kept and part_plan_wc takes 64-byte sectors (17
    slots): a cost, recorded in DESIGN.md §4.  The grids weigh 113 .. 236 MB (T = 100) and 639 MB (T = 40000: 7.1e7 cells of 9 bytes,
    aggregate only); 2e4 rows each."""
    pl = plan_tiles(K, T)
    n = 20000
    wc = plan_wc(pl, n, False, "wc")
    assert (pl.shift_part, pl.nparts, pl.n_chunks, wc.sec) == B2_CASES[(K, T)]
    if pl.nparts == LINE_PARTS:
        assert plan_wc(pl, n, False, "auto").sec == 8 and plan_wc(pl, n, False, "auto").cap == 16 and (LDS_BUDGET - 16) // 986 == 161
    k, t, v = random_rows(n, K, T, seed=T + K % 1000)
    k[1] = (pl.nparts - 1) * pl.KP
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"), aggs=("svc", ""), jobs=(("EWMA", "svc"),) if T == 100 else ())


def test_unforced_write_combining_rules(engine):
    """part_plan_wc under partition_pass = auto, the only plan decision the engine shows (stage0_path 2 against 3): the mean-arrivals
    rule `2 * 1024 / nparts > cap - (sec - 1)` on either side (41 and 42 partitions of 128 keys), the issue's pair 512 x 64 (refused)
    and 40000 x 100 (taken); the `>= 24 records per run` rule is searched for over every partition count and found unreachable."""
    for nparts in range(1, MAX_PARTS + 1):
        for has2 in (False, True):
            pl = SimpleNamespace(nparts=nparts, rpt=next(r for r in SORT_RPT if r * THREADS * (2 if has2 else 1) * 10 + (nparts + 4) * 16 + 64 <= LDS_BUDGET))
            per = (LDS_BUDGET - 16) // nparts
            if per >= WC_FIXED + 72 and (per - WC_FIXED) // 8 < 18:                    # 64-byte sectors without being forced
                assert pl.rpt * THREADS * (2 if has2 else 1) // nparts < 24
    for K, T, nparts, taken in ((512, 64, 2, False), (40000, 100, 313, True), (128 * 41, 100, 41, False), (128 * 41 + 1, 100, 42, True)):
        pl = plan_tiles(K, T)
        n = 30000
        wc = plan_wc(pl, n, False, "auto")
        assert pl.nparts == nparts and (wc is not None) == taken
        if K == 40000:
            assert (wc.cap, wc.sec, wc.rpt) == (61, 16, 4)
        k, t, v = random_rows(n, K, T, seed=K)
        dense_checks(engine, k, t, v, K, pl, passes=("auto",), aggs=("svc",))


def _planted(K, T, cb, variant, seed):
    """3000 rows + on (key K - 1, bucket T - 1), (key 0, bucket 0) and (key 1, bucket T / 2): three rows of 2^(64 - cb) - 1 (they stay in
    the record) and, in the variant `over`, two rows of 2^(64 - cb) (the overflow list)"""
    limit = 1 << (64 - cb)
    k, t, v = random_rows(3000, K, T, seed=seed)
    cells = [(K - 1, T - 1), (0, 0), (1, T // 2)]
    vals = [limit - 1] * 3 + ([limit, limit] if variant == "over" else [limit - 2])
    k = np.concatenate([k, np.repeat(np.array([c[0] for c in cells], dtype=U64), len(vals))])
    t = np.concatenate([t, T0 + np.repeat(np.array([c[1] for c in cells], dtype=np.int64), len(vals))])
    v = np.concatenate([v, np.tile(np.array(vals, dtype=U64), 3)])
    o = np.random.default_rng(seed).permutation(k.size)
    return k[o], t[o], v[o], limit


@pytest.mark.parametrize("variant", ["fits", "over"])
@pytest.mark.parametrize("T,cb", [(32766, 15), (32767, 16), (65535, 17)])
def test_record_cell_and_value_fields(engine, T, cb, variant):
    """part_plan_tiles: cell_bits is bumped when 2^cb - 1 <= KP * T (the all-ones cell is reserved); pass B: value_limit = 2^(64 - cb).
    K = 3: KP 1, the largest cell T - 1 = 32765 of 15 bits, then 16 and 17 bits.  Several planted rows share a point, so the overflow
    list's fold and the tile meet in one grid cell: under `max` the maximum is the record's in `fits` and the list's in `over`."""
    K = 3
    pl = plan_tiles(K, T)
    assert (pl.KP, pl.nparts, pl.cell_bits) == (1, 3, cb) and ((1 << cb) - 1 > T) and (cb == 15 or (1 << (cb - 1)) - 1 <= T)
    k, t, v, limit = _planted(K, T, cb, variant, seed=T)
    assert limit == pl.value_limit and int((v >= U64(limit)).sum()) == (6 if variant == "over" else 0) and int((v == U64(limit - 1)).sum()) == 9
    pk, pt, pv = orc.stage0(k, t, v, "max")
    assert int(pv[-1]) == (limit if variant == "over" else limit - 1) and (int(pk[-1]), int(pt[-1])) == (K - 1, T0 + T - 1)
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"))


@pytest.mark.parametrize("T,dense", [(65535, True), (65536, False)])
def test_tile_plan_ends_at_65536_buckets(engine, T, dense):
    """part_plan_tiles / tad_capi_job.cpp (stage0_dense): T >= 2^16 has no tile plan, the direct scatter runs (path 1, in one attempt)"""
    K = 2
    pl = plan_tiles(K, T)
    assert (pl is not None) == dense
    k, t, v = random_rows(2000, K, T, seed=T)
    assert lattice(t)[1:] == (1, T)
    with engine.plan(partition_pass="wc", **DENSE):
        res, _ = check_job(engine, "EWMA", k, t, v, K, agg_flow="svc")
        assert (res.stats["stage0_path"], res.stats["stage0_attempts"], res.stats["n_buckets"]) == (3 if dense else 1, 1, T)
        agg_check(engine, k, t, v, K, "", (3 if dense else 1,))


@pytest.mark.parametrize("step,mode", [(1, 0), (65538, 1), (65539, 2)])
def test_lattice_modes_at_the_32_bit_edge(engine, step, mode):
    """make_lattice / lattice_bucket / the fast path of pass B: mode 0 (step 1), mode 1 (multiply-high, exact for d < 2^32: the last bucket
    at d = 2^32 - 4), mode 2 (division, the GENERIC kernels) when (nb - 1) * step > 2^32 - 1.  Rows on buckets 0, 1, T - 2, T - 1, so
    the gcd is the step.  Derived, hinted, and hinted one bucket too short (a second attempt, the same rows)."""
    K, T = 2, 65535
    assert lattice_mode(step, T) == mode
    assert (T - 1) * 65538 == (1 << 32) - 4 and (T - 1) * 65539 > (1 << 32) - 1
    rng = np.random.default_rng(step)
    bucket = np.tile(np.array([0, 1, T - 2, T - 1], dtype=np.int64), 50)
    k = rng.integers(0, K, size=bucket.size).astype(U64)
    k[:8] = (0, 0, 0, 0, 1, 1, 1, 1)
    t = T0 + step * bucket
    v = rng.integers(1, 3_000_000_000, size=bucket.size).astype(U64)
    assert lattice(t) == (T0, step, T)
    pl = plan_tiles(K, T)
    assert (pl.KP, pl.n_chunks, pl.tb) == (1, 4, 16384)
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"))
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"), lattice=(T0, step, T))
    dense_checks(engine, k, t, v, K, pl, passes=("wc",), aggs=("svc",), attempts=2, lattice=(T0, step, T - 1))


# ================================================================== C. pass B
def ragged_keys(k, n, chunk, tile, K, spare):
    """the rows of every chunk's ragged last tile get keys from the `spare` highest key ids, which occur nowhere else"""
    r = np.arange(n, dtype=np.int64)
    ragged = (r % chunk) >= (chunk // tile) * tile
    k = np.where(ragged, U64(K - spare) + (r.astype(U64) % U64(spare)), k % U64(K - spare))
    return k, ragged


WC_CHUNKS = (2046, 2048, 2050, 4094, 4096, 4098, 6144, 6146)


@pytest.mark.parametrize("chunk", WC_CHUNKS)
def test_wc_chunks_at_tile_edges(engine, chunk):
    """k_partition_wc: tiles of RPT * 1024 rows, nfull whole tiles by 16-byte loads and one ragged tile, two register sets
    (load_tile(tile + 2)), the counter pairs by tile parity.  RPT 2 (2000 x 100: 16 partitions; two-sided): 1 to 4 tiles; RPT 4
    (40000 x 100: 313 partitions): 1 and 2.  The rows of the ragged tile carry keys seen nowhere else."""
    n = G * chunk
    for K, T, has2, rpt in ((2000, 100, False, 2), (2000, 100, True, 2), (40000, 100, False, 4)):
        pl = plan_tiles(K, T, has2)
        wc = plan_wc(pl, n * (2 if has2 else 1), has2, "wc")
        tile = wc.rpt * THREADS
        assert wc.rpt == rpt and plan_bins(n, K).chunk == chunk and pl.nparts == (16 if K == 2000 else 313)
        k, t, v = orc.synth_rows(chunk, n, K, T)
        k, ragged = ragged_keys(k, n, chunk, tile, K, 64)
        assert int(ragged.sum()) == G * (chunk % tile) and ceil_div(chunk, tile) == {2: {2046: 1, 2048: 1, 2050: 2, 4094: 2, 4096: 2, 4098: 3, 6144: 3, 6146: 4},
                                                                                       4: {2046: 1, 2048: 1, 2050: 1, 4094: 1, 4096: 1, 4098: 2, 6144: 2, 6146: 2}}[rpt][chunk]
        k2 = None
        if has2:
            k2 = np.where(ragged, k, (k * U64(7) + U64(3)) % U64(K - 64))
            k2[::10] = SKIP
        dense_checks(engine, k, t, v, K, pl, passes=("wc",), aggs=("pod" if has2 else "svc",), jobs=(("EWMA", "svc"),) if rpt == 2 and not has2 else (), k2=k2)


@pytest.mark.parametrize("chunk,has2,generic", [(c, False, True) for c in (4094, 4096, 4098, 8192)] + [(c, True, False) for c in (4094, 4096, 4098)] +
                         [(c, False, False) for c in (10238, 10240, 10242)])
def test_sort_chunks_at_tile_edges(engine, chunk, has2, generic):
    """k_partition: tiles of rpt * 1024 rows — 10240 one-sided, 4096 two-sided (part_plan_tiles: 8 rows x 2 sides do not fit LDS) and
    4096 for the GENERIC kernels (an end_time) — nfull whole tiles, one ragged tile with guarded loads"""
    K, T = 2000, 100
    n = G * chunk
    pl = plan_tiles(K, T, has2)
    tile = sort_tile_rows(pl, has2, generic)
    assert pl.rpt == (4 if has2 else 10) and tile == (10240 if not (has2 or generic) else 4096) and plan_bins(n, K).chunk == chunk
    k, t, v = orc.synth_rows(chunk, n, K, T)
    k, ragged = ragged_keys(k, n, chunk, tile, K, 64)
    assert int(ragged.sum()) == G * (chunk % tile)
    k2 = None
    if has2:
        k2 = np.where(ragged, k, (k * U64(7) + U64(3)) % U64(K - 64))
        k2[::10] = SKIP
    kw = dict(end_time=int(t.max()) + 1) if generic else {}
    dense_checks(engine, k, t, v, K, pl, passes=("sort",), aggs=("pod" if has2 else "svc",), jobs=(("EWMA", "pod" if has2 else "svc"),) if chunk < 8192 else (), k2=k2, **kw)


def tile_position(i):
    """place i of a list over tile 0 of a chunk (RPT 2): consecutive places go to different wavefront steps.  Step j of wavefront w holds
    the rows 2 * (64 w + lane) + j: 32 steps of 64 lanes in 2048 rows"""
    grp, lane = i % 32, i // 32
    return 2 * (64 * (grp >> 1) + lane) + (grp & 1)


def lanes_per_step(parts_of_tile):
    """the most lanes of one wavefront step of a 2048-row tile (RPT 2) on one partition"""
    p = np.asarray(parts_of_tile, dtype=np.int64)
    pos = np.arange(p.size)
    step = ((pos >> 1) >> 6) * 2 + (pos & 1)
    return int(np.bincount(step * (int(p.max()) + 1) + p).max())


@functools.lru_cache(maxsize=None)
def flat_table(P, KP, m, tile0, seed):
    """a flat table: every workgroup's chunk (P * m rows) holds exactly m rows of every partition, so every histogram row is flat and
    every queue has the plan's depth.  tile0: ((partition, records), ...) of the first 2048 rows of every chunk; the other partitions share
    the rest of that tile evenly.  -> partition of every row of one chunk"""
    tile0 = dict(tile0)
    rest = [p for p in range(P) if p not in tile0]
    fill = 2048 - sum(tile0.values())
    counts = dict(tile0)
    for i, p in enumerate(rest):
        counts[p] = fill // len(rest) + (i < fill % len(rest))
    assert sum(counts.values()) == 2048 and max(counts.values()) <= m
    first = np.concatenate([np.full(c, p) for p, c in sorted(counts.items())])
    tile = np.empty(2048, dtype=np.int64)
    tile[[tile_position(i) for i in range(2048)]] = first
    later = np.concatenate([np.full(m - counts[p], p) for p in range(P)])
    later = later[np.random.default_rng(seed).permutation(later.size)]
    return np.concatenate([tile, later])


def flat_rows(P, KP, T, chunk_parts, seed):
    n = G * chunk_parts.size
    rng = np.random.default_rng(seed)
    k = (np.tile(chunk_parts, G) * KP + rng.integers(0, KP, size=n)).astype(U64)
    sec = rng.integers(0, T, size=n).astype(np.int64)
    sec[:2] = (0, T - 1)
    return k, T0 + sec, rng.integers(1, 3_000_000_000, size=n).astype(U64)


def assert_flat(k, pl, wc, chunk):
    """lines 903-904 of k_partition_wc: `skewed` is false for every workgroup, so every queue is wc_cap deep"""
    hist = np.bincount((np.arange(k.size) // chunk) * pl.nparts + (k >> U64(pl.shift_part)).astype(np.int64), minlength=G * pl.nparts).reshape(G, pl.nparts)
    regions = (hist + wc.sec - 1) & ~(wc.sec - 1)
    rmax, rsum, ract = regions.max(axis=1), regions.sum(axis=1), (regions != 0).sum(axis=1)
    assert not ((rmax * pl.nparts * 2 > rsum * 3) | (ract * 4 < pl.nparts * 3)).any()


@pytest.mark.parametrize("pp", ["wc", "wc_sectors"])
def test_wc_queue_fill_levels(engine, pp):
    """k_partition_wc's append and emit: `pos == SEC - 1` registers the queue, `pos < qc` or the record spills, `whole = c & ~(SEC - 1)`,
    the remainder slides down, leftovers and fillers at the end.  In tile 0 of every workgroup partition j receives exactly a_j of
    {SEC - 1, SEC, SEC + 1, 2 SEC - 1, 2 SEC, cap - 1, cap, cap + 1} records, never 8 lanes of one wavefront step."""
    P, KP, T, m = 64, 128, 100, 96
    K = P * KP
    pl = plan_tiles(K, T)
    n = G * P * m
    wc = plan_wc(pl, n, False, pp)
    assert (pl.nparts, pl.KP, wc.rpt) == (P, KP, 2) and (wc.sec, wc.cap) == ((16, 64) if pp == "wc" else (8, 16))
    levels = [wc.sec - 1, wc.sec, wc.sec + 1, 2 * wc.sec - 1, 2 * wc.sec, wc.cap - 1, wc.cap, wc.cap + 1]
    parts = flat_table(P, KP, m, tuple((j, a) for j, a in enumerate(levels)), 7)
    assert np.bincount(parts, minlength=P).tolist() == [m] * P and np.bincount(parts[:2048], minlength=P)[:8].tolist() == levels
    assert lanes_per_step(parts[:2048]) < WAVE_AGG_MIN
    k, t, v = flat_rows(P, KP, T, parts, 8)
    assert plan_bins(n, K).chunk == parts.size
    assert_flat(k, pl, wc, parts.size)
    dense_checks(engine, k, t, v, K, pl, passes=(pp,), hists=("exact", "sampled"))


@pytest.mark.parametrize("variant", ["288", "289", "1792"])
def test_wc_parks_288_spills_and_stores_the_289th(engine, variant):
    """k_partition_wc: kSpillSlots = 288 records that found their queue full are parked per tile and stored in the emit phase; the 289th
    is stored directly.  Three partitions receive cap + 96 records in tile 0 (288 spills), one of them one more (289); 16 partitions
    x 128 records per tile on a plan with cap 16 (1792 spills)."""
    T, KP = 100, 128
    if variant == "1792":
        P, m, pp, tile0 = 16, 128, "wc_sectors", tuple((p, 128) for p in range(16))
    else:
        P, m, pp = 48, 176, "wc"
        tile0 = ((3, 64 + 96), (20, 64 + 96), (47, 64 + 96 + (variant == "289")))
    K = P * KP
    pl = plan_tiles(K, T)
    n = G * P * m
    wc = plan_wc(pl, n, False, pp)
    assert (pl.nparts, wc.rpt, wc.cap) == (P, 2, 16 if variant == "1792" else 64)
    parts = flat_table(P, KP, m, tile0, 9)
    first = np.bincount(parts[:2048], minlength=P)
    assert int(np.maximum(first - wc.cap, 0).sum()) == int(variant) and (int(variant) > SPILL_SLOTS) == (variant != "288")
    assert lanes_per_step(parts[:2048]) < WAVE_AGG_MIN and n <= 2_700_000
    k, t, v = flat_rows(P, KP, T, parts, 10)
    assert_flat(k, pl, wc, parts.size)
    dense_checks(engine, k, t, v, K, pl, passes=(pp,), jobs=(("EWMA", "svc"),) if variant != "1792" else ())


WAVE_VARIANTS = ("seven", "eight", "first_lane_odd", "all", "two_groups")


def wave_step(variant, A, B):
    """partitions of the 64 lanes of one wavefront step; the other lanes sit on >= 48 different partitions, none of them A or B"""
    others = [p for p in range(64) if p not in (A, B)]
    lanes = np.array(others[:62] + others[:2])
    if variant == "seven":
        lanes[:7] = A
    elif variant == "eight":
        lanes[:8] = A
    elif variant == "first_lane_odd":          # the first lane holds the odd row out: the LAST lane's group is asked
        lanes[0], lanes[56:] = B, A
    elif variant == "all":
        lanes[:] = A
    else:                                      # two groups of 8: only the first lane's is taken together, the other one queues
        lanes[:8], lanes[8:16] = A, B
    return lanes


def test_wave_aggregation_at_7_and_8_lanes(engine):
    """k_partition_wc / hist_add: lanes of a wavefront step on one partition (one histogram bin) are handled together from
    kWaveAggMin = 8 on; if the first lane's group is smaller the last active lane's group is asked.  Chunks of 128 rows: workgroup g's
    wavefront 0 holds its even rows in step 0 (variant g % 5) and its odd rows in step 1 (64 different partitions)."""
    P, KP, T, chunk = 64, 128, 100, 128
    K, n = P * KP, G * chunk
    pl = plan_tiles(K, T)
    assert (pl.nparts, pl.KP, pl.shift_bin) == (P, KP, 0) and plan_bins(n, K).chunk == chunk
    rng = np.random.default_rng(12)
    parts = np.empty((G, chunk), dtype=np.int64)
    for g in range(G):
        A, B = (5 + g) % 64, (37 + g) % 64
        parts[g, 0::2] = wave_step(WAVE_VARIANTS[g % 5], A, B)
        parts[g, 1::2] = rng.permutation(64)
        cnt = np.bincount(parts[g, 0::2], minlength=64)
        want = {"seven": (7, 2), "eight": (8, 2), "first_lane_odd": (8, 2), "all": (64, 0), "two_groups": (8, 8)}[WAVE_VARIANTS[g % 5]]
        assert int(cnt[A]) == want[0] and int(np.delete(cnt, A).max()) <= want[1] and (WAVE_VARIANTS[g % 5] != "two_groups" or cnt[B] == 8)
        assert (cnt[A] >= WAVE_AGG_MIN) == (WAVE_VARIANTS[g % 5] != "seven") and (WAVE_VARIANTS[g % 5] != "first_lane_odd" or parts[g, 0] != parts[g, 126] == A)
        assert WAVE_VARIANTS[g % 5] == "all" or np.unique(parts[g, 0::2]).size >= 48
    parts = parts.ravel()
    k = (parts * KP + 5 + (np.arange(n) % 2) * rng.integers(0, 100, size=n)).astype(U64)      # step 0: one key, so one histogram bin, per partition
    sec = rng.integers(0, T, size=n).astype(np.int64)
    sec[:2] = (0, T - 1)
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    dense_checks(engine, k, T0 + sec, v, K, pl, passes=PASSES, hists=("exact", "sampled"))


# ================================================================== D. pass C
@functools.lru_cache(maxsize=None)
def split_table(records, hot_key):
    """K = 300, T = 64: partitions of 256 and 44 keys.  `records` rows in the partition of hot_key, 1000 in the other.  50000 of the hot
    partition's rows sit on ONE point with values of [2^48, 2^49): their sum wraps mod 2^64; the last input row is that point's maximum"""
    rng = np.random.default_rng(records + hot_key)
    K, T = 300, 64
    lo, hi = (0, 256) if hot_key < 256 else (256, 300)
    olo, ohi = (256, 300) if hot_key < 256 else (0, 256)
    rest = records - 50000
    k = np.concatenate([rng.integers(lo, hi, size=rest), np.full(50000, hot_key), rng.integers(olo, ohi, size=1000)]).astype(U64)
    sec = np.concatenate([rng.integers(0, T, size=rest), np.full(50000, 13), rng.integers(0, T, size=1000)]).astype(np.int64)
    v = rng.integers(1, 3_000_000_000, size=k.size).astype(U64)
    v[rest:records] = rng.integers(1 << 48, (1 << 49) - 1, size=50000).astype(U64)
    v[rest] = U64((1 << 49) - 1)                                  # the point's maximum ...
    k[0], sec[0], sec[-1] = lo, 0, T - 1
    o = rng.permutation(k.size)
    o = np.concatenate([o[o != rest], [rest]])                    # ... is the last input row
    k, sec, v = k[o], sec[o], v[o]
    return np.ascontiguousarray(k), T0 + sec, np.ascontiguousarray(v), K, T


@pytest.mark.parametrize("records,hot_key", [(131071, 7), (131072, 7), (131073, 7), (262144, 7), (262145, 7), (131073, 290)])
def test_slice_split_at_exactly_2_17_records(engine, records, hot_key):
    """k_part_offsets / k_part_tail / pass C: `tot > slice_len` splits a partition, its grid tile is pre-zeroed (`k < g.K`: the partial
    last partition with hot key 290) and its slices merge with atomics.  Sort pass and exact histogram: no fillers, tot is the row
    count.  slice_len = max(2^17, 1.5 x the mean partition): 2^17 for the three sizes around it; with 262144 records beside 1000 the
    mean partition is 131572 and a slice 197358, so those two sizes sit inside the rule (two slices), not on it.  The same tables run
    under wc and under the sampled layout (slices of 3 * 2^17: one slice)."""
    k, t, v, K, T = split_table(records, hot_key)
    pl = plan_tiles(K, T)
    tot = np.bincount((k >> U64(pl.shift_part)).astype(np.int64), minlength=2)
    hot = 0 if hot_key < 256 else 1
    assert (pl.KP, pl.nparts) == (256, 2) and tot[hot] == records and tot[1 - hot] == 1000 and lattice(t)[1:] == (1, T)
    sl = slice_len_of(False, k.size, pl.nparts)
    assert sl == (SLICE_RECORDS if records < 200000 else 197358) and slice_len_of(True, k.size, pl.nparts) == 3 * SLICE_RECORDS
    assert ceil_div(records, sl) == (1 if records <= SLICE_RECORDS else 2) and (records > sl) == (records > SLICE_RECORDS)
    pk, pt, pv = orc.stage0(k, t, v, "sum")
    point = (pk == U64(hot_key)) & (pt == T0 + 13)
    assert int(np.sum(v[(k == U64(hot_key)) & (t == T0 + 13)].astype(object))) >= 1 << 64 and int(v[-1]) == int(v.max()) and point.sum() == 1
    dense_checks(engine, k, t, v, K, pl, passes=("sort",))
    dense_checks(engine, k, t, v, K, pl, passes=("wc",), jobs=())
    dense_checks(engine, k, t, v, K, pl, passes=("sort",), hists=("sampled",), jobs=())


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 8704, 8705])
def test_tile_walk_at_wavefront_chunk_edges(engine, rows):
    """k_tile_aggregate's exact walk: a wavefront takes 512 consecutive records (`i + 7 * 64 < hi`), then one ragged chunk.  One
    partition, sort pass: the records are the rows, workgroup by workgroup.  The order inside a workgroup is the order its LDS atomics
    land in, so EVERY row of the last workgroup with rows is the only row of its point: whichever record is last, dropped, a point
    is missing."""
    K, T = 200, 64
    pl = plan_tiles(K, T)
    chunk = plan_bins(rows, K).chunk
    assert (pl.KP, pl.nparts) == (256, 1)
    last_lo = (ceil_div(rows, chunk) - 1) * chunk
    rng = np.random.default_rng(rows)
    k = rng.integers(0, 100, size=rows).astype(U64)
    sec = rng.integers(0, T, size=rows).astype(np.int64)
    nl = rows - last_lo
    k[last_lo:] = 100 + np.arange(nl) % 100                                     # keys 100 .. 199 occur in the last workgroup only
    sec[last_lo:] = 1 + np.arange(nl) // 100
    k[0], sec[0] = (0, 0) if rows > 1 else (k[0], sec[0])
    t = T0 + sec
    v = rng.integers(1, 3_000_000_000, size=rows).astype(U64)
    pk, pt, _ = orc.stage0(k, t, v, "sum")
    assert int((pk >= U64(100)).sum()) == nl and nl <= chunk
    whole = rows // (64 * WALK_U)
    assert (rows % (64 * WALK_U) == 0) == (rows in (512, 8192, 8704)) and whole == {1: 0, 63: 0, 64: 0, 65: 0, 511: 0, 512: 1, 513: 1, 8191: 15, 8192: 16, 8193: 16, 8704: 17, 8705: 17}[rows]
    dense_checks(engine, k, t, v, K, pl, passes=("sort",))


#           K, T: (KP, n_chunks, tb)
D3_CASES = {(5, 17744): (1, 1, 17744), (5, 17745): (1, 2, 8873), (3, 8872): (2, 1, 8872), (3, 8873): (1, 1, 8873),
            (7, 65535): (1, 4, 16384), (8, 65535): (1, 4, 16384), (9, 65535): (1, 4, 16384), (17, 65535): (1, 4, 16384)}


@pytest.mark.parametrize("K,T", sorted(D3_CASES))
def test_bucket_rounds_and_their_workgroup_ids(engine, K, T):
    """k_tile_aggregate's bucket rounds: tb = ceil(T / n_chunks), the last round short (`b_lo + tb <= T`), `c = cg - c_lo` wrapping for
    the cells of earlier rounds, the rounds as parallel workgroups with s_idx = (y / n_chunks) * 8 + x (7, 8, 9 and 17 partitions of one
    key: slices on either side of a row of 8 block ids).  Every key has rows on buckets r * tb - 1, r * tb and T - 1 for every round."""
    pl = plan_tiles(K, T)
    assert (pl.KP, pl.n_chunks, pl.tb) == D3_CASES[(K, T)] and pl.nparts == ceil_div(K, pl.KP)
    assert pl.tb * pl.n_chunks >= T > pl.tb * (pl.n_chunks - 1) and (T == 65535) == (T - pl.tb * (pl.n_chunks - 1) == 16383)
    edges = sorted({0, T - 1} | {r * pl.tb - 1 for r in range(1, pl.n_chunks)} | {r * pl.tb for r in range(1, pl.n_chunks)})
    pts = [(key, edges, 2) for key in range(K)] + [(key, np.random.default_rng(key).integers(0, T, size=40), 1) for key in range(K)]
    k, t, v = rows_on(pts, seed=K + T)
    assert lattice(t)[1:] == (1, T)
    dense_checks(engine, k, t, v, K, pl, passes=("sort", "wc"))


#           K, T: (KP, bucket rounds, narrow (kt, rounds), wide (kt, rounds))
D4_CASES = {(1000, 17): (1024, 1, (1024, 1), (512, 2)), (1000, 69): (256, 1, (256, 1), (128, 2)), (262272, 100): (512, 3, (256, 2), (171, 3))}


@functools.lru_cache(maxsize=None)
def settle_table(K, T):
    pl = plan_tiles(K, T)
    n = 30 * K if K <= 1000 else 300_000
    k, t, v = orc.synth_rows(3, n, K, T)
    v = v.copy()
    noise, edge = set(), []
    for narrow in (True, False):
        kt, rounds = plan_settle(pl, T, narrow)
        for part in (0, pl.nparts - 1):
            for r in range(1, rounds + 1):
                for key in (part * pl.KP + r * kt - 1, part * pl.KP + r * kt):          # the last key of a round and the first of the next
                    if key < K:
                        noise.add(key)
                if narrow:
                    edge.append(part * pl.KP + min(r * kt, K - part * pl.KP) - 1)
    noise.add(K - 1)
    extra_k, extra_t, extra_v = [], [], []
    for key in sorted(noise):                                                          # a full series with one spike: a noise point
        extra_k += [key] * T
        extra_t += list(orc.SYNTH_T_BASE + 60 * np.arange(T))
        extra_v += [2_000_000_000] * (T - 1) + [40_000_000_000]
    k = np.concatenate([k, np.array(extra_k, dtype=U64)])
    t = np.concatenate([t, np.array(extra_t, dtype=np.int64)])
    v = np.concatenate([v, np.array(extra_v, dtype=U64)])
    return k, t, v, sorted(noise), sorted(set(e for e in edge if e < K))


@pytest.mark.parametrize("tile_cells", ["auto", "wide"])
@pytest.mark.parametrize("K,T", sorted(D4_CASES))
def test_settle_rounds_and_narrow_cells_at_their_edges(engine, K, T, tile_cells):
    """part_plan_settle / pass C in settle mode (DBSCAN, anomalies only; emit_all takes the bucket rounds): kt keys per round, balanced;
    narrow cells (`max`) hold value + 1, narrow_limit = 2^32 - 2; the bitmap window of 40 words from (k0 + chunk * kt) & ~31.  A noise
    key as the last key of every round and the first of the next, key K - 1 in a partial last partition; under `max` values of
    2^32 - 3, 2^32 - 2 and 2^32 - 1 on the last key of a round, and 2^(64 - cb) - 1 and 2^(64 - cb) on key K - 1."""
    pl = plan_tiles(K, T)
    KP, chunks, narrow, wide = D4_CASES[(K, T)]
    assert (pl.KP, pl.n_chunks, plan_settle(pl, T, True), plan_settle(pl, T, False)) == (KP, chunks, narrow, wide)
    assert K % pl.KP != 0 and (K != 262272 or wide[0] % 32 != 0)
    k, t, v, noise, edge = settle_table(K, T)
    v = v.copy()
    sec = (t - orc.SYNTH_T_BASE) // 60
    for key in edge:                                                                   # the narrow cell's last value, the sentinel, one beyond
        for b, val in ((1, NARROW_LIMIT - 1), (2, NARROW_LIMIT), (3, NARROW_LIMIT + 1)):
            v[(k == U64(key)) & (sec == b)] = U64(val)
    v[(k == U64(K - 1)) & (sec == 5)] = U64(pl.value_limit - 1)
    v[(k == U64(K - 1)) & (sec == 6)] = U64(pl.value_limit)
    assert int((v == U64(NARROW_LIMIT)).sum()) >= len(edge) > 0 and int((v >= U64(pl.value_limit)).sum()) >= 1
    passes = ("sort", "wc") if K <= 1000 else ("wc",)
    for agg in ("", "svc"):
        want = orc.run_job("DBSCAN", k, t, v, agg_flow=agg)
        assert set(noise) <= set(want["key_id"].tolist())
        for p in passes:
            with engine.plan(partition_pass=p, tile_cells=tile_cells, **DENSE):
                res, _ = job_check(engine, "DBSCAN", k, t, v, K, agg, want=want)
                assert res.stats["stage0_path"] == expected_path(pl, k.size, False, p) and res.stats["stage0_attempts"] == 1
                assert (res.stats["n_buckets"], res.stats["step"], res.stats["rows_used"]) == (T, 60, k.size)


@pytest.mark.parametrize("extra", [0, 1])
def test_overflow_list_exactly_full(engine, extra):
    """pass B / k_apply_overflow: `o < kOverflowCap` (2^20).  1 048 576 rows >= 2^49 among 1.1e6: the list is exactly full, path 2 / 3 in
    one attempt; one entry more raises DEV_ERR_OVERFLOW_LIST and the direct scatter redoes the job (path 1, two attempts).  Both give
    the oracle's rows; 70000 overflow rows share one point (a sum that wraps, a max)."""
    K, T, n = 64, 32, 1_100_000
    big = OVERFLOW_CAP + extra
    k, t, v = orc.synth_rows(0, n, K, T)
    v = v.copy()
    pl = plan_tiles(K, T)
    assert pl.cell_bits == 15 and pl.value_limit == 1 << 49
    v[:big] = U64(1 << 49) + np.arange(big, dtype=U64) * U64(1 << 28)
    k[:70000], t[:70000] = 9, orc.SYNTH_T_BASE + 60 * 7
    v[:70000] = U64(1 << 60) + np.arange(70000, dtype=U64)
    assert int((v >= U64(pl.value_limit)).sum()) == big and 70000 * (1 << 60) >= 1 << 64
    want = {agg: orc.run_job("EWMA", k, t, v, agg_flow=agg) for agg in ("svc", "")}
    for p in ("sort", "wc"):
        path = expected_path(pl, n, False, p)
        with engine.plan(partition_pass=p, **DENSE):
            for agg in ("svc", ""):
                res = engine.run("EWMA", k, t, v, K, agg_flow=agg)
                assert (res.stats["stage0_path"], res.stats["stage0_attempts"]) == ((1, 2) if extra else (path, 1))
                assert res.n_rows == want[agg]["n_anomalies"] and res.stats["rows_used"] == n and res.stats["n_points"] == want[agg]["n_points"]
                for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
                    assert (res[f] == want[agg][f]).all(), f
            agg_check(engine, k, t, v, K, "svc", (1,) if extra else (path,), want=want["svc"]["points"])
