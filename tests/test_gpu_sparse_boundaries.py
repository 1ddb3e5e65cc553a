"""GPU: the sparse Stage 0 (tad_sparse.hip) at every tile, round and record-width edge, bit for bit against the CPU oracle
(DESIGN.md §4 has the table):
  A  the LSD radix sort: tiles of 4096 slots with a short last one, wavefront slices of 512, runs of equal (key, time) that cross
     tile edges and meet in the output through 64-bit atomics, the balanced digit plans (1 .. 5 passes, both start buffers), the
     filtered slots (key field K) that must sort last, crowded and flat digit histograms
  B  the partition pass + LDS sort: rounds of <= 14336 records (k_ss_plan), split sets of 8192 (k_ss_split), the MSD bucket rule
     and mshift (k_ss_sort), the fold across threads of 14 slots, the one-pass / three-pass output, the rank-grid transposition in
     chunks of 4096 staged points (k_ss_place), the record's cell and value bits (part_plan_sparse, pass B)
  C  the rule that sends a table to the sparse path at all (tad_capi_job.cpp: choose_stage0)

References: orc.stage0 (a numpy group-by) for engine.aggregate, orc.run_job for the rows of engine.run with and without emit_all,
through the check helpers of tests/test_gpu_sparse.py and tests/test_gpu_sparse_partition.py.  No tolerances anywhere.

Every case asserts from host-side numbers that it sits on the edge it is named for BEFORE the engine is asked: sorted-slot
positions from np.unique over the composite (key, time), the partition plan and k_ss_plan's greedy rounds from the few lines of
Python below, and afterwards what the engine exposes (stage0_path, stage0_attempts, n_buckets, step).

What cannot be seen from outside and is therefore never relied on: pass B's filler records (a block's exact record-slot count)
and the order of the rows of ONE point inside a sorted round (the LDS counting sort places equal keys in the order its atomics
land).  A case that plants a maximum "in the first / a middle / the last piece" of a run does so exactly for the LSD sort, which is
stable; for the partition sort it plants it on the first / a middle / the last input row of the point.
A sum over one LDS round cannot wrap mod 2^64 on the partition path: a record holds values below 2^(64 - cell_bits) <= 2^49 and
a round 14336 records (< 2^63 in all); the cases use sums far beyond the record's value field instead (the fold is 64-bit).

The builders are plain functions of seeded numpy, usable without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import tad_oracle as orc
from job_helpers import PART, check_lsd, check_part, class_boundary_table, lattice

pytestmark = pytest.mark.gpu

# the constants of the kernels and plans, mirrored (a change there must be followed here)
RS_TILE = 4096                # tad_sparse.hip:220   kRsTile = kRsThreads * kRsItems: slots per workgroup of the LSD sort
RS_WAVE_SLOTS = 512           # tad_sparse.hip:286   64 * kRsItems: consecutive slots a wavefront of k_rs_scatter ranks
RS_DIGIT = 8                  # tad_sparse.hip:459   np = ceil(bits / 8) balanced digits
RS_MAX_TB = 32                # tad_sparse.hip:457   time bits capped at 32
SPARSE_MIN_CELLS = 1 << 24    # choose_stage0        sparse iff cells >= 2^24 && slots < cells / 8 (or the grid does not fit)
SPARSE_FILL = 8               # choose_stage0
SS_ITEMS = 14                 # tad_sparse.hip:566   kSsItems: sorted slots a thread of k_ss_sort folds
SS_CAP = 14336                # tad_sparse.hip:567   kSsCap = 1024 * 14 records per LDS round
SPLIT_SET = 8192              # tad_sparse.hip:671   kSet = kSplitThreads * 2 * kL records per set of k_ss_split
SS_MSD_BITS = 13              # tad_sparse.hip:717   kSsMsdBits
SS_MAX_BUCKET = 32            # tad_sparse.hip:718   kSsMaxBucket
SS_ONE_PASS_BYTES = 20        # tad_sparse.hip:999   one_pass iff U * 20 <= kSsCap * 8  (U <= 5734)
SP_THREADS = 1024             # tad_sparse.hip:1057  kSpThreads: dr = 1024 / range
SP_CHUNK = 4096               # tad_sparse.hip:1058  kSpChunk staged points per step of k_ss_place
MAX_BINS = 16384              # tad_internal.h:560   kMaxBins (part_plan_bins: bins of one key for K <= 16384)
SECTOR_PARTS = (156 * 1024) // (8 * 9 + 18)     # tad_stage0_part.hip:1571  kLdsBudget / 90 = 1774 key blocks at most
MIN_CELL_BITS = 15            # tad_stage0_part.hip:53, :1577
MAX_SPARSE_CELL_BITS = 28     # tad_stage0_part.hip:1576  shift_part + bit_width(T) above this: the plan refuses, the LSD sort runs
WC_MAX_FILL = 15 * 256        # tad_stage0_part.hip:1650  at most (sec - 1) fillers per (workgroup, key block), sec <= 16, G = 256

T0 = 1660202814
U64 = np.uint64
SKIP = orc.KEY_SKIP
LSD = dict(sparse="always", sparse_sort="lsd")
DENSE_PATHS = (1, 2, 3)
assert SS_CAP * 8 // SS_ONE_PASS_BYTES == 5734


# ------------------------------------------------------------------ shared helpers
def agg_check(engine, k, t, v, K, agg, paths, k2=None):
    """engine.aggregate against the numpy group-by"""
    pk, pt, pv = orc.stage0(k, t, v, "sum" if agg else "max", k2)
    pts = engine.aggregate(k, t, v, K, agg_flow=agg, key_id2=k2)
    assert pts.stats["stage0_path"] in paths, pts.stats["stage0_path"]
    assert pts.n_points == pk.size == pts.stats["n_points"]
    assert (pts["key_id"] == pk).all() and (pts["flow_end_s"] == pt).all() and (pts["value"] == pv).all()
    return pts


def sorted_slots(k, t, K, k2=None):
    """the LSD sort's slots in sorted order -> (composite key << 32 | t - t0 with key K for a filtered slot, input slot of every sorted
    slot).  Slot of (row i, side h) = i * sides + h (k_sparse_keys); the sort is stable."""
    keys = k if k2 is None else np.stack([k, k2], axis=1).ravel()
    tt = t if k2 is None else np.repeat(t, 2)
    live = keys != SKIP
    dt = (tt - tt[live].min()).astype(U64)
    comp = np.where(live, (np.where(live, keys, U64(0)) << U64(32)) | dt, U64(K) << U64(32))
    order = np.argsort(comp, kind="stable")
    return comp[order], order


def run_edges(comp, K):
    """first slot, last slot of every run of equal live (key, time) in the sorted order, and the number of live slots"""
    live = comp[(comp >> U64(32)) < U64(K)]
    _, first, cnt = np.unique(live, return_index=True, return_counts=True)
    return first, first + cnt - 1, int(live.size)


def rs_plan(K, span):
    """rs_plan of tad_sparse.hip:454 -> (time bits, bits, digit widths)"""
    tb = min(int(span).bit_length(), RS_MAX_TB)
    bits = tb + int(K).bit_length()                      # K itself must sort: the filtered slots
    n = max(1, (bits + RS_DIGIT - 1) // RS_DIGIT)
    widths, left = [], bits
    for i in range(n):
        w = max(1, (left + (n - i) - 1) // (n - i))
        widths.append(w)
        left -= w
    return tb, bits, widths


def part_plan(K, T):
    """part_plan_bins (tad_stage0_part.hip:1484) + part_plan_sparse (:1565)"""
    sb = 0
    while -(-K // (1 << sb)) > MAX_BINS:
        sb += 1
    parts = lambda c: -(-K // (1 << c))
    sp = sb
    while sp < 13 and parts(sp) > SECTOR_PARTS:
        sp += 1
    tbits = int(T).bit_length()
    return SimpleNamespace(shift_bin=sb, shift_part=sp, KP=1 << sp, nparts=parts(sp), bins_per_part=1 << (sp - sb), tbits=tbits,
                           cell_bits=max(MIN_CELL_BITS, sp + tbits), fits=parts(sp) <= SECTOR_PARTS and sp + tbits <= MAX_SPARSE_CELL_BITS)


def block_rounds(pl, k, block):
    """k_ss_plan (tad_sparse.hip:593) for one key block: [(key0, key1, records)] — whole bins, greedily, acc + c <= SS_CAP"""
    k = k[k != SKIP].astype(np.int64)
    kb = k[(k >> pl.shift_part) == block]
    counts = np.bincount((kb & (pl.KP - 1)) >> pl.shift_bin, minlength=pl.bins_per_part)
    out, acc, first = [], 0, 0
    for b, c in enumerate(counts):
        c = int(c)
        if acc != 0 and acc + c > SS_CAP:
            out.append((first << pl.shift_bin, b << pl.shift_bin, acc))
            acc = 0
        if acc == 0:
            first = b
        acc += c
    if acc != 0:
        out.append((first << pl.shift_bin, pl.KP, acc))
    return out, int(counts.max(initial=0))


def round_sort(pl, k, t, block, rnd):
    """k_ss_sort's view of one round: (bits, mshift, largest MSD bucket, unique points) from its sort keys key-in-round << tbits | bucket"""
    key0, key1, n = rnd
    live = k != SKIP
    t0, step, _ = lattice(t[live])
    kk = k.astype(np.int64)
    kib = kk & (pl.KP - 1)
    m = live & ((kk >> pl.shift_part) == block) & (kib >= key0) & (kib < key1)
    assert int(m.sum()) == n
    sk = ((kib[m] - key0) << pl.tbits) | ((t[m] - t0) // step)
    kbits = int(key1 - key0 - 1).bit_length()
    bits = pl.tbits + kbits
    mshift = bits - min(bits, SS_MSD_BITS)
    return SimpleNamespace(bits=bits, mshift=mshift, max_bucket=int(np.bincount(sk >> mshift).max()), U=int(np.unique(sk).size), sk=np.sort(sk))


def table(points, seed, vlo=1, vhi=3_000_000_000, shuffle=True):
    """points: [(key, bucket array, rows per point: int or array)] -> key, time, value columns, rows in a seeded arbitrary order"""
    kk, tt = [], []
    for key, b, r in points:
        b = np.asarray(b, dtype=np.int64)
        kk.append(np.repeat(np.full(b.size, key, dtype=U64), r))
        tt.append(np.repeat(b, r))
    k, t = np.concatenate(kk), T0 + np.concatenate(tt)
    rng = np.random.default_rng(seed)
    v = rng.integers(vlo, vhi, size=k.size).astype(U64)
    o = rng.permutation(k.size) if shuffle else np.arange(k.size)
    return np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o])


def spread(n, span, seed):
    """n distinct buckets of [0, span), sorted"""
    return np.sort(np.random.default_rng(seed).choice(span, size=n, replace=False))


# ================================================================== A. the LSD radix sort
A1_SLOTS = (1, 2, 63, 64, 65, RS_WAVE_SLOTS - 1, RS_WAVE_SLOTS, RS_WAVE_SLOTS + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1,
            2 * RS_TILE - 1, 2 * RS_TILE, 2 * RS_TILE + 1, 3 * RS_TILE + 1)
A1_CASES = [(s, s, False) for s in A1_SLOTS] + [(2 * n, 2 * n, True) for n in (2047, 2048, 2049)] + \
           [(s, f, False) for s in A1_SLOTS for f in (4095, 4096, 4097) if f < s] + [(4098, 4095, True), (4098, 4096, True), (4098, 4097, True)]


@functools.lru_cache(maxsize=None)
def slots_table(slots, live, two):
    """`slots` row slots (rows x sides) on 37 keys and 600 seconds, slots - live of them filtered out (TAD_KEY_SKIP)"""
    rng = np.random.default_rng(1000 + slots * 3 + live)
    sides = 2 if two else 1
    n = slots // sides
    keys = rng.integers(0, 37, size=slots).astype(U64)
    keys[rng.permutation(np.arange(2 if two else 0, slots))[:slots - live]] = SKIP      # (two sides: the first row stays live on both)
    keys = keys.reshape(n, sides)
    t = T0 + rng.integers(0, 600, size=n).astype(np.int64)
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    return np.ascontiguousarray(keys[:, 0]), (np.ascontiguousarray(keys[:, 1]) if two else None), t, v


@pytest.mark.parametrize("slots,live,two", A1_CASES)
def test_lsd_slot_counts_at_tile_and_wavefront_edges(engine, slots, live, two):
    """k_rs_hist / k_rs_scatter / k_rs_heads / k_rs_reduce: n_tile of the last tile, `in == false` lanes inside a ballot, and the first
    filtered slot of the sorted order on either side of the first tile edge"""
    K = 37
    k, k2, t, v = slots_table(slots, live, two)
    comp, _ = sorted_slots(k, t, K, k2)
    _, _, n_live = run_edges(comp, K)
    assert comp.size == slots and n_live == live
    if live != slots:
        first_filtered = int(np.flatnonzero((comp >> U64(32)) == U64(K))[0])
        assert first_filtered == live and abs(first_filtered - RS_TILE) <= 1
    agg = "pod" if two else "svc"
    with engine.plan(**LSD):
        agg_check(engine, k, t, v, K, agg, (4, 7), k2)
        kw = dict(key_id2=k2) if two else {}
        check_lsd(engine, "EWMA", k, t, v, K, agg, **kw)


def _tile_run_sizes(variant, tail):
    sizes, named, pos = [], {}, 0

    def small(upto):
        nonlocal pos
        i = 0
        while pos < upto:
            s = min(1 + i % 3, upto - pos)
            sizes.append(s)
            pos += s
            i += 1

    def run(name, n):
        nonlocal pos
        named[name] = (pos, pos + n - 1)
        sizes.append(n)
        pos += n

    if variant == "split":
        small(4090); run("ends_4095", 6); run("starts_4096", 5)
    else:
        small(4095); run("straddles", 2)
    small(2 * RS_TILE); run("whole_tile", RS_TILE)
    small(12300); run("long", 12400)
    if tail == "short":
        small(24990); run("last", 10)                      # 25000 slots: the last tile holds 424
    else:
        small(7 * RS_TILE - 12); run("last", 12)           # the live slots end on a tile edge, filtered ones follow
    return sizes, named, pos


@functools.lru_cache(maxsize=None)
def tile_run_table(variant, tail):
    """runs of equal (key, time) laid out in sorted order by _tile_run_sizes; run i is (key i // 97, second i % 97); rows shuffled"""
    sizes, named, n_live = _tile_run_sizes(variant, tail)
    rng = np.random.default_rng(7)
    idx = np.repeat(np.arange(len(sizes)), sizes)
    k = (idx // 97).astype(U64)
    t = T0 + (idx % 97).astype(np.int64)
    K = len(sizes) // 97 + 1
    if tail == "edge":
        k = np.concatenate([k, np.full(100, SKIP, dtype=U64)])
        t = np.concatenate([t, T0 + rng.integers(0, 97, size=100)])
    o = rng.permutation(k.size)
    return np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), K, named, n_live


def _assert_tile_runs(k, t, K, variant, tail, named, n_live):
    comp, order = sorted_slots(k, t, K)
    first, last, live = run_edges(comp, K)
    has = lambda a, b: bool(((first == a) & (last == b)).any())
    assert live == n_live
    if variant == "split":
        assert RS_TILE - 1 in last and RS_TILE in first
    else:
        assert has(RS_TILE - 1, RS_TILE)
    assert has(2 * RS_TILE, 3 * RS_TILE - 1)                                     # exactly one whole tile
    assert has(12300, 24699) and not ((first > 12300) & (first < 24700)).any()
    assert 12300 // RS_TILE == 3 and 24699 // RS_TILE == 6                       # tiles 4 and 5 lie inside the run: no head of their own
    assert int(last.max()) == live - 1
    if tail == "short":
        assert comp.size == live and live % RS_TILE != 0
    else:
        assert live % RS_TILE == 0 and comp.size == live + 100
    for name, (a, b) in named.items():
        assert has(a, b), name
    return order


@pytest.mark.parametrize("variant,tail", [("split", "short"), ("straddle", "edge"), ("split", "edge"), ("straddle", "short")])
def test_lsd_runs_across_tile_edges_sum(engine, variant, tail):
    """k_rs_zero / k_rs_reduce with wrapping add: values near 2^63, so the pieces of a run wrap mod 2^64 when they meet"""
    k, t, K, named, n_live = tile_run_table(variant, tail)
    _assert_tile_runs(k, t, K, variant, tail, named, n_live)
    v = (U64(1 << 63) + np.random.default_rng(8).integers(0, 1000, size=k.size).astype(U64))
    with engine.plan(**LSD):
        agg_check(engine, k, t, v, K, "svc", (4, 7))
        if tail == "short":
            check_lsd(engine, "EWMA", k, t, v, K, "svc")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("variant,tail", [("split", "short"), ("straddle", "edge")])
def test_lsd_runs_across_tile_edges_max(engine, variant, tail, where):
    """unsigned max: a run's maximum planted in its first, a middle (a tile without a head of its own) and its last tile"""
    k, t, K, named, n_live = tile_run_table(variant, tail)
    order = _assert_tile_runs(k, t, K, variant, tail, named, n_live)
    v = np.random.default_rng(9).integers(1, 1_000_000_000, size=k.size).astype(U64)
    a, b = named["long"]
    slot = {"first": a + 5, "middle": 4 * RS_TILE + 1616, "last": b - 3}[where]
    assert slot // RS_TILE == {"first": 3, "middle": 4, "last": 6}[where]
    v[order[slot]] = U64(1 << 40)                                                 # the stable sort puts this input row on `slot`
    if variant == "straddle":
        v[order[RS_TILE - 1 if where == "first" else RS_TILE]] = U64(1 << 41)
    with engine.plan(**LSD):
        agg_check(engine, k, t, v, K, "", (4, 7))
        if where == "middle":
            check_lsd(engine, "EWMA", k, t, v, K, "")


#            K, span, step, bits, digit widths
A3_CASES = [(1, 127, 1, 8, [8]),
            (1, 128, 1, 9, [5, 4]),
            (255, 255, 1, 16, [8, 8]),
            (256, 255, 1, 17, [6, 6, 5]),
            (4095, 4095, 1, 24, [8, 8, 8]),
            (4096, 4095, 1, 25, [7, 6, 6, 6]),
            (32767, 7 * 18000, 7, 32, [8, 8, 8, 8]),
            (1, (1 << 31) + 5, 1, 33, [7, 7, 7, 6, 6]),
            (65536, (1 << 16) - 1, 1, 33, [7, 7, 7, 6, 6])]


@functools.lru_cache(maxsize=None)
def digit_table(K, span, step):
    """~9000 rows over three tiles: keys over all of [0, K) with K - 1 present, times over the whole lattice with both ends present, 300
    filtered rows (their key field K must sort behind K - 1)"""
    rng = np.random.default_rng(K * 31 + span % 1000)
    n = 9001
    k = rng.integers(0, K, size=n).astype(U64)
    k[:40] = K - 1
    t = step * rng.integers(0, span // step + 1, size=n).astype(np.int64)
    t[0], t[1] = 0, span
    k[rng.permutation(np.arange(3, n))[:300]] = SKIP
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    return k, T0 + t, v


@pytest.mark.parametrize("K,span,step,bits,widths", A3_CASES)
def test_lsd_digit_plans(engine, K, span, step, bits, widths):
    """rs_plan: bits = bit_width(span) + bit_width(K); 1 .. 5 balanced digits; the parity of the pass count picks the start buffer"""
    k, t, v = digit_table(K, span, step)
    live = k != SKIP
    t0, st, nb = lattice(t[live])
    assert (st, (nb - 1) * st) == (step, span) and int(k[live].max()) == K - 1 and int((~live).sum()) == 300
    tb, got_bits, got_widths = rs_plan(K, span)
    assert (got_bits, got_widths) == (bits, widths) and sum(widths) == bits and len(widths) == -(-bits // 8)
    assert 2 * RS_TILE < k.size <= 3 * RS_TILE
    comp, _ = sorted_slots(k, t, K)
    assert ((comp[-300:] >> U64(32)) == U64(K)).all() and int(comp[-301] >> U64(32)) == K - 1      # K behind K - 1
    with engine.plan(**LSD):
        pts = agg_check(engine, k, t, v, K, "svc", (4, 7))
        assert pts.stats["n_buckets"] == nb and pts.stats["step"] == step
        res, _ = check_lsd(engine, "EWMA", k, t, v, K, "svc")
        assert res.stats["n_buckets"] == nb and res.stats["step"] == step and res.stats["stage0_attempts"] == 1


def test_lsd_crowded_and_flat_digit_histograms(engine):
    """pass 0 reads the rows in input order: tile 0 has one lowest digit on all 4096 slots (one LDS counter, ranks up to 4095), tile 1
    every one of the 256 digits exactly 16 times"""
    K = 255
    rng = np.random.default_rng(41)
    k = np.concatenate([np.arange(RS_TILE) % K, rng.integers(0, K, size=RS_TILE)]).astype(U64)
    sec = np.concatenate([np.full(RS_TILE, 7), rng.permutation(np.arange(RS_TILE) % 256)]).astype(np.int64)
    t = T0 + sec
    v = rng.integers(1, 3_000_000_000, size=k.size).astype(U64)
    tb, bits, widths = rs_plan(K, 255)
    assert lattice(t) == (T0, 1, 256) and (tb, widths) == (8, [8, 8])
    digit0 = (t - T0) & 255                                                       # rs_digit at shift 0, mask 255: the time field
    digit1 = k.astype(np.int64)                                                   # at shift 8: the key
    assert (np.bincount(digit0[:RS_TILE], minlength=256) == np.where(np.arange(256) == 7, RS_TILE, 0)).all()
    assert np.unique(digit1[:RS_TILE]).size == K
    assert (np.bincount(digit0[RS_TILE:], minlength=256) == 16).all()
    with engine.plan(**LSD):
        agg_check(engine, k, t, v, K, "svc", (4, 7))
        agg_check(engine, k, t, v, K, "", (4, 7))
        check_lsd(engine, "EWMA", k, t, v, K, "svc")


# ================================================================== B. the partition pass + LDS sort
def _part_checks(engine, k, t, v, K, T, algos=(("EWMA", "svc"),), aggs=("svc", "")):
    """under PART: the jobs on path 8 in one attempt, the aggregates on path 8 / 10"""
    out = None
    with engine.plan(**PART):
        for algo, agg in algos:
            res, _ = check_part(engine, algo, k, t, v, K, agg)
            assert res.stats["stage0_attempts"] == 1 and res.stats["n_buckets"] == T
            out = res if out is None else out
        for agg in aggs:
            agg_check(engine, k, t, v, K, agg, (8, 10))
    return out


@functools.lru_cache(maxsize=None)
def round_table():
    """K = 3000: key blocks of two keys, bins of one key.  Every heavy block has empty blocks on either side."""
    day = 16000
    pts = [(200, np.arange(SS_CAP), 1),                                            # block 100: one key of exactly 14336 distinct points, alone
           (400, spread(SS_CAP - 100, day, 1), 1), (401, spread(100, day, 2), 1),   # block 200: 14236 + 100 = one exactly full round
           (600, spread(SS_CAP - 100, day, 3), 1), (601, spread(101, day, 4), 1),   # block 300: one record more: two rounds
           (800, spread(SS_CAP // 2, day, 5), 2), (801, [777], 1),                  # block 400: a full round and a round of one record
           (1000, spread(5734, day, 6), 2),                                         # block 500: U = 5734 at two rows per point: one_pass
           (1200, spread(5735, day, 7), 2),                                         # block 600: U = 5735: three passes through LDS
           (0, [0, day - 1], 1), (2999, [0, day - 1], 1)]
    return table(pts, seed=50) + (3000, day)


def test_part_round_capacity_and_output_form(engine):
    """k_ss_plan: acc + c <= 14336; k_ss_sort's output: one_pass iff U <= 5734; a full round of 14336 distinct points"""
    k, t, v, K, T = round_table()
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and (pl.shift_bin, pl.KP, pl.nparts, pl.bins_per_part, pl.cell_bits, pl.fits) == (0, 2, 1500, 2, 15, True)
    want = {100: [(0, 2, SS_CAP)], 200: [(0, 2, SS_CAP)], 300: [(0, 1, SS_CAP - 100), (1, 2, 101)], 400: [(0, 1, SS_CAP), (1, 2, 1)],
            500: [(0, 2, 11468)], 600: [(0, 2, 11470)]}
    for block, rounds in want.items():
        assert block_rounds(pl, k, block)[0] == rounds, block
        for side in (block - 1, block + 1):
            assert block_rounds(pl, k, side)[0] == []
    assert round_sort(pl, k, t, 100, want[100][0]).U == SS_CAP
    u1, u2 = round_sort(pl, k, t, 500, want[500][0]).U, round_sort(pl, k, t, 600, want[600][0]).U
    assert (u1, u2) == (5734, 5735) and u1 * SS_ONE_PASS_BYTES <= SS_CAP * 8 < u2 * SS_ONE_PASS_BYTES
    _part_checks(engine, k, t, v, K, T)


def test_part_round_of_14337_records_goes_to_the_lsd_sort(engine):
    """a bin above kSsCap raises DEV_ERR_SPARSE_ROUND: the same rows from the LSD sort, in a second attempt"""
    day = 16000
    k, t, v = table([(200, np.arange(SS_CAP + 1), 1), (0, [0, day - 1], 1), (2999, [0, day - 1], 1)], seed=51)
    pl = part_plan(3000, day)
    rounds, biggest = block_rounds(pl, k, 100)
    assert pl.fits and biggest == SS_CAP + 1 and rounds == [(0, 1, SS_CAP + 1)]      # (the greedy rule closes the oversized bin's round at the next bin)
    with engine.plan(**PART):
        res, _ = check_part(engine, "EWMA", k, t, v, 3000, "svc", paths=(4,))
        assert res.stats["stage0_attempts"] == 2
        agg_check(engine, k, t, v, 3000, "svc", (4, 7))


@functools.lru_cache(maxsize=None)
def bucket_table(extra):
    """K = 7000: key blocks of 4 keys, T = 86400.  Block 50: its four keys have 40 points each far apart (one per 512 seconds), key 201
    also has 32 consecutive seconds inside the aligned 64-second window [6400, 6464).  extra: one more row of value 0 on one of them."""
    rng = np.random.default_rng(52)
    far = lambda s: 512 * spread(40, 160, s) + 17
    pts = [(200 + j, far(60 + j), 1) for j in range(4)] + [(201, 6400 + np.arange(32), 1), (0, [0, 86399], 1), (6999, [5, 86399], 1)]
    pts += [(int(key), spread(6, 86400, 70 + int(key)), 1) for key in rng.choice(np.arange(300, 6900), size=60, replace=False)]
    k, t, v = table(pts, seed=53)
    if extra:
        k, t, v = np.append(k, U64(201)), np.append(t, T0 + 6420), np.append(v, U64(0))
    return k, t, v, 7000, 86400


@pytest.mark.parametrize("algo,agg", [("EWMA", "svc"), ("DBSCAN", "")])
def test_part_msd_bucket_of_32_and_33(engine, algo, agg):
    """k_ss_sort: a round whose largest MSD bucket holds exactly 32 records is put in order by counting inside the buckets, one of 33 by
    the stable LSD passes.  The 33rd record is a second row of value 0 on an existing point: both ways must give the same rows."""
    got = []
    for extra, occupancy in ((False, SS_MAX_BUCKET), (True, SS_MAX_BUCKET + 1)):
        k, t, v, K, T = bucket_table(extra)
        pl = part_plan(K, T)
        assert lattice(t)[1:] == (1, T) and (pl.KP, pl.tbits, pl.cell_bits, pl.fits) == (4, 17, 19, True)
        rounds, _ = block_rounds(pl, k, 50)
        assert rounds == [(0, 4, 4 * 40 + 32 + extra)]                              # the round spans the block's KP keys
        s = round_sort(pl, k, t, 50, rounds[0])
        assert (s.bits, s.mshift, s.max_bucket) == (19, 6, occupancy)               # a bucket = 64 consecutive seconds of one key
        with engine.plan(**PART):
            res, _ = check_part(engine, algo, k, t, v, K, agg)
            assert res.stats["stage0_attempts"] == 1 and res.stats["n_buckets"] == T
            got.append(agg_check(engine, k, t, v, K, agg, (8, 10)))
    for f in ("key_id", "flow_end_s", "value"):
        assert (got[0][f] == got[1][f]).all(), f


@pytest.mark.parametrize("T,bits,mshift", [(5000, 13, 0), (10000, 14, 1)])
def test_part_mshift_0_and_1_with_100_rows_on_one_point(engine, T, bits, mshift):
    """bits == 13: the MSD counting sort is the whole sort (no order inside a bucket: a bucket IS one point, however crowded);
    bits == 14: two points share a bucket, and the crowded one sends the round to the LSD passes"""
    K = 1000
    b = spread(300, T, 54)
    k, t, v = table([(7, b, 1), (7, [b[150]], 100), (7, [b[150] ^ 1], 3), (0, [0, T - 1], 1), (999, [T - 1], 2)], seed=55)
    pl = part_plan(K, T)
    rounds, _ = block_rounds(pl, k, 7)
    s = round_sort(pl, k, t, 7, rounds[0])
    assert lattice(t)[1:] == (1, T) and pl.KP == 1 and len(rounds) == 1 and (s.bits, s.mshift) == (bits, mshift)
    assert s.max_bucket >= 101 > SS_MAX_BUCKET
    _part_checks(engine, k, t, v, K, T, algos=(("EWMA", "svc"), ("DBSCAN", "")))


FOLD_R = (1, 13, 14, 15, 27, 28, 29, 42, 43, 200)


@functools.lru_cache(maxsize=None)
def fold_table():
    """K = 1000 (a key block is one key).  Key 7: one round whose sorted order is known — bits < 13, so the sort key decides every slot
    but the order of one point's rows: points of r rows, each r starting on a sorted slot = 0, 1 and 13 (mod 14), single-row points between.
    Key 9: one point of 14336 rows.  -> (k, t, K, T, rows per point of key 7 in time order)"""
    rows, pos = [], 0
    for m in (0, 1, 13):
        for r in FOLD_R:
            while pos % SS_ITEMS != m:
                rows.append(1)
                pos += 1
            rows.append(r)
            pos += r
    rows = np.array(rows)
    T = rows.size
    kk = np.concatenate([np.repeat(np.full(T, 7, dtype=U64), rows), np.full(SS_CAP, 9, dtype=U64), np.array([0, 999], dtype=U64)])
    tt = T0 + np.concatenate([np.repeat(np.arange(T), rows), np.full(SS_CAP, 5), [0, T - 1]]).astype(np.int64)
    o = np.random.default_rng(56).permutation(kk.size)
    return np.ascontiguousarray(kk[o]), np.ascontiguousarray(tt[o]), 1000, T, rows


def _assert_fold(k, t, K, T, rows):
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and pl.KP == 1 and pl.cell_bits == 15 and pl.tbits + 0 < SS_MSD_BITS
    r7, _ = block_rounds(pl, k, 7)
    r9, _ = block_rounds(pl, k, 9)
    assert r7 == [(0, 1, int(rows.sum()))] and r9 == [(0, 1, SS_CAP)]
    s = round_sort(pl, k, t, 7, r7[0])
    sk, first, cnt = np.unique(s.sk, return_index=True, return_counts=True)       # the oracle's counts: every point's first sorted slot
    assert s.mshift == 0 and (cnt == rows).all()
    seen = {(int(c), int(f) % SS_ITEMS) for f, c in zip(first, cnt)}
    assert seen >= {(r, m) for r in FOLD_R for m in (0, 1, 13)}
    assert round_sort(pl, k, t, 9, r9[0]).U == 1                                   # every thread behind thread 0: a lead, no head
    return pl


def test_part_fold_across_threads_sum(engine):
    """the s_lead / s_lflag chain with wrapping add: sums far beyond the record's 49 value bits (the fold is 64-bit)"""
    k, t, K, T, rows = fold_table()
    pl = _assert_fold(k, t, K, T, rows)
    limit = 1 << (64 - pl.cell_bits)
    v = np.random.default_rng(57).integers(limit // 2, limit, size=k.size).astype(U64)
    assert int(v.max()) < limit and SS_CAP * (limit // 2) > limit
    _part_checks(engine, k, t, v, K, T, aggs=("svc",))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_part_fold_across_threads_max(engine, where):
    """unsigned max: the one maximum of the 14336-row point, of the 200-row points and of the 43-row points on the first, a middle and
    the last of the point's input rows (wherever the sort puts it: the head's own slots or some thread's lead).  The three variants
    only SAMPLE positions of the chain: none is known to hit the head's own 14 slots; the sum case above carries the chain rule, since
    there every lead counts"""
    k, t, K, T, rows = fold_table()
    pl = _assert_fold(k, t, K, T, rows)
    v = np.random.default_rng(58).integers(1, 1 << 40, size=k.size).astype(U64)
    big = U64((1 << (64 - pl.cell_bits)) - 1)
    sec = t - T0
    targets = [(k == 9)] + [(k == 7) & (sec == b) for b in np.flatnonzero(rows >= 43)]
    for m in targets:
        idx = np.flatnonzero(m)
        v[idx[{"first": 0, "middle": idx.size // 2, "last": idx.size - 1}[where]]] = big
    with engine.plan(**PART):
        agg_check(engine, k, t, v, K, "", (8, 10))
        if where == "middle":
            res, _ = check_part(engine, "EWMA", k, t, v, K, "")
            assert res.stats["stage0_attempts"] == 1


@functools.lru_cache(maxsize=None)
def split_table():
    """K = 10000: key blocks of 8 keys (8 bins).  Six blocks, their records and rounds:
    block 10: 4001 (odd), 1 round, 1 set | 20: 12000 (even), 1 round, 2 sets | 30: 2 x 10000, 2 rounds, 3 sets |
    40: 9500 + 9500 + 9000, 3 rounds, 4 sets | 50: 4 x 7200, 4 rounds, 4 sets | 60: 5 x 7200, 5 rounds, 5 sets"""
    T = 6000
    spec = {10: [500] * 7 + [501], 20: [1500] * 8, 30: [10000, 0, 0, 10000], 40: [9500, 0, 9500, 0, 0, 9000],
            50: [7200, 7200, 0, 7200, 7200], 60: [0, 7200, 7200, 7200, 7200, 0, 7200]}
    pts = [(0, [0, T - 1], 1), (9999, [0, T - 1], 1)]
    for block, sizes in spec.items():
        for j, n in enumerate(sizes):
            if n:
                pts.append((block * 8 + j, spread(n // 2, T, block + j), 2))      # two rows per point
                if n % 2:
                    pts.append((block * 8 + j, [T // 2], 1))
    return table(pts, seed=59) + (10000, T, spec)


def test_part_split_sets_and_round_counts(engine):
    """k_ss_split: 1 .. 5 sets of 8192 records loaded two ahead in pairs, 1 .. 5 rounds per block (rbits 0 .. 3 ballots per record).  Pass B
    adds up to 15 fillers per (workgroup, block): every block sits well inside its class of sets"""
    k, t, v, K, T, spec = split_table()
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and (pl.KP, pl.bins_per_part, pl.nparts, pl.fits) == (8, 8, 1250, True)
    want = {10: (4001, 1, 1), 20: (12000, 1, 2), 30: (20000, 2, 3), 40: (28000, 3, 4), 50: (28800, 4, 4), 60: (36000, 5, 5)}
    seen_rbits = set()
    for block, (records, n_rounds, sets) in want.items():
        rounds, biggest = block_rounds(pl, k, block)
        assert sum(r[2] for r in rounds) == records == sum(spec[block]) and len(rounds) == n_rounds and biggest <= SS_CAP
        assert -(-records // SPLIT_SET) == sets == -(-(records + WC_MAX_FILL) // SPLIT_SET)         # fillers cannot change the class
        seen_rbits.add((n_rounds - 1).bit_length())
    assert seen_rbits == {0, 1, 2, 3} and want[10][0] % 2 == 1 and want[20][0] % 2 == 0
    _part_checks(engine, k, t, v, K, T, aggs=("svc",))


@functools.lru_cache(maxsize=None)
def place_table():
    """K = 3000 (blocks of two keys), one point per row.  Staged points of the blocks' single rounds:
    block 100: 4095 + 1 (U = 4096, the second key's first point is staged point 4095) | 200: 4096 + 1 (U = 4097, the second key starts on
    point 4096) | 300: 4095 | 400: 9000 points of one key: three chunks | 500: 4000 + 4193 (U = 8193: the second key spans both chunk edges)"""
    T = 10000
    pts = [(200, spread(4095, T, 1), 1), (201, [4242], 1), (400, spread(4096, T, 2), 1), (401, [17], 1), (600, spread(4095, T, 3), 1),
           (801, spread(9000, T, 4), 1), (1000, spread(4000, T, 5), 1), (1001, spread(4193, T, 6), 1), (0, [0, T - 1], 1), (2999, [0, T - 1], 1)]
    return table(pts, seed=60) + (3000, T)


def test_part_rank_grid_transposition_chunk_edges(engine):
    """k_ss_place: chunks of 4096 staged points; a key's series begins, ends or continues at a chunk edge (`j == 0 || rk == 0`)"""
    k, t, v, K, T = place_table()
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and pl.KP == 2 and pl.fits
    pk, _, _ = orc.stage0(k, t, v, "sum")
    staged = {}
    for block, U in ((100, 4096), (200, 4097), (300, 4095), (400, 9000), (500, 8193)):
        rounds, _ = block_rounds(pl, k, block)
        assert len(rounds) == 1
        keys = pk[(pk >> U64(1)) == U64(block)]                                     # the round's staged points, in order
        assert keys.size == U == round_sort(pl, k, t, block, rounds[0]).U
        staged[block] = keys
    assert {U for U in map(len, staged.values())} == {SP_CHUNK - 1, SP_CHUNK, SP_CHUNK + 1, 2 * SP_CHUNK + 1, 9000}
    assert int(np.flatnonzero(staged[100] == U64(201))[0]) == SP_CHUNK - 1        # first point = staged point 4095
    assert int(np.flatnonzero(staged[200] == U64(401))[0]) == SP_CHUNK            # starts on point 4096
    assert (staged[400] == U64(801)).all() and -(-9000 // SP_CHUNK) == 3
    a = int(np.flatnonzero(staged[500] == U64(1001))[0])
    assert a < SP_CHUNK and staged[500][2 * SP_CHUNK] == U64(1001)                  # continues over both chunk edges
    _part_checks(engine, k, t, v, K, T)


@functools.lru_cache(maxsize=None)
def wide_block_table():
    """K = 2^21 keys, ~5e4 rows on second-resolution timestamps, at most 8 points per key"""
    rng = np.random.default_rng(61)
    K = 1 << 21
    keys = np.sort(rng.choice(K, size=12000, replace=False))
    keys[0], keys[-1] = 0, K - 1
    n_k = rng.integers(1, 9, size=keys.size)
    pts = [(int(key), spread(int(n), 86400, int(key) % 9973), 1) for key, n in zip(keys, n_k)] + [(0, [0], 2), (K - 1, [86399], 3)]
    k, t, v = table(pts, seed=62)
    return k, t, v, K, 86400


def test_part_blocks_of_more_than_1024_keys(engine):
    """K = 2^21: bins of 128 keys, key blocks of 2048 keys: k_ss_place's dr = 1024 / range is 0, every step of its walk wraps the key"""
    k, t, v, K, T = wide_block_table()
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and 1 << pl.shift_bin == 128 and pl.KP == 2048 and pl.bins_per_part == 16 and pl.cell_bits == 28 and pl.fits
    pk, _, _ = orc.stage0(k, t, v, "max")
    assert int(np.bincount((pk >> U64(7)).astype(np.int64)).max()) <= SS_CAP and np.unique(pk, return_counts=True)[1].max() <= 9
    ranges = [r[1] - r[0] for block in range(0, pl.nparts, 97) for r in block_rounds(pl, k, block)[0]]
    assert ranges and max(ranges) > SP_THREADS and SP_THREADS // max(ranges) == 0
    _part_checks(engine, k, t, v, K, T, algos=(("DBSCAN", ""),), aggs=("",))


@pytest.mark.parametrize("algo,agg", [("EWMA", "svc"), ("DBSCAN", "")])
def test_part_length_classes_at_every_class_boundary(engine, algo, agg):
    """k_ss_compact feeding the length classes (path 9): series of 16 / 64 / 256 points and their neighbours"""
    k, t, v, K = class_boundary_table()
    with engine.plan(sparse_classes="always", **PART):
        check_part(engine, algo, k, t, v, K, agg, paths=(9,))
        agg_check(engine, k, t, v, K, agg, (10,))


@pytest.mark.parametrize("T", [5000, 86400])
def test_part_record_value_field(engine, T):
    """pass B: a value of 2^(64 - cell_bits) - 1 fits the record (and the point's 64-bit sum leaves the field behind); one more raises
    DEV_ERR_OVERFLOW_LIST and the LSD sort redoes the job"""
    K = 3000
    pl = part_plan(K, T)
    assert pl.fits and pl.cell_bits == {5000: 15, 86400: 18}[T]
    limit = 1 << (64 - pl.cell_bits)
    pts = [(int(key), spread(5, T, int(key)), 2) for key in range(100, 2900, 37)] + [(0, [0, T - 1], 1), (2999, [0, T - 1], 1)]
    k, t, v = table(pts, seed=63)
    rows = np.flatnonzero((k == U64(1025)) & (t == t[k == U64(1025)].min()))
    extra = np.full(5, U64(limit - 1))
    k1, t1, v1 = np.append(k, np.full(5, U64(1025))), np.append(t, np.full(5, t[rows[0]])), np.append(v, extra)
    assert lattice(t1)[1:] == (1, T) and int(v1.max()) == limit - 1 and 5 * (limit - 1) > limit
    _part_checks(engine, k1, t1, v1, K, T)
    v2 = v1.copy()
    v2[-1] = U64(limit)
    with engine.plan(**PART):
        res, _ = check_part(engine, "EWMA", k1, t1, v2, K, "svc", paths=(4,))
        assert res.stats["stage0_attempts"] == 2
        agg_check(engine, k1, t1, v2, K, "", (4, 7))


@pytest.mark.parametrize("tbits,path", [(27, 8), (28, 4)])
def test_part_cell_bits_28_and_29(engine, tbits, path):
    """part_plan_sparse: shift_part + bit_width(T) == 28 takes the partition form, 29 the LSD sort — refused by the plan, so in one attempt"""
    K = 3000
    T = (1 << (tbits - 1)) + 1
    rng = np.random.default_rng(64)
    k = rng.integers(0, K, size=3000).astype(U64)
    sec = rng.integers(0, T, size=3000).astype(np.int64)
    sec[:3] = (0, T - 1, 1)
    k[:3] = (0, K - 1, 1)
    t = T0 + sec
    v = rng.integers(1, 3_000_000_000, size=3000).astype(U64)
    pl = part_plan(K, T)
    assert lattice(t)[1:] == (1, T) and pl.shift_part == 1 and pl.tbits == tbits and pl.fits == (path == 8)
    with engine.plan(**PART):
        res, _ = check_part(engine, "EWMA", k, t, v, K, "svc", paths=(path,))
        assert res.stats["stage0_attempts"] == 1 and res.stats["n_buckets"] == T
        agg_check(engine, k, t, v, K, "svc", (8, 10) if path == 8 else (4, 7))


@pytest.mark.parametrize("T", [(1 << 14) - 1, 1 << 14])
def test_part_last_bucket_of_the_last_key_of_a_block(engine, T):
    """the largest cell of a block, (T - 1) * KP + KP - 1, at T = 2^k - 1 and 2^k: the record's all-ones cell belongs to the fillers"""
    K = 3000
    pl = part_plan(K, T)
    assert pl.KP == 2 and pl.fits and pl.cell_bits == {16383: 15, 16384: 16}[T]
    assert (T - 1) * pl.KP + pl.KP - 1 < (1 << pl.cell_bits) - 1
    pts = [(int(key), spread(6, T - 1, int(key)), 2) for key in range(100, 2900, 53)]
    pts += [(201, [T - 1], 3), (201, [0], 2), (200, [T - 1], 2), (2999, [T - 1, 0], 2), (0, [0, T - 1], 1)]
    k, t, v = table(pts, seed=65)
    assert lattice(t)[1:] == (1, T)
    _part_checks(engine, k, t, v, K, T, algos=(("EWMA", "svc"), ("DBSCAN", "")))


# ================================================================== C. the sparse rule itself
@functools.lru_cache(maxsize=None)
def rule_table(T, n):
    rng = np.random.default_rng(T + n % 1000)
    K = 4096
    k = rng.integers(0, K, size=n).astype(U64)
    sec = rng.integers(0, T, size=n).astype(np.int64)
    sec[:3] = (0, T - 1, 1)
    v = rng.integers(1, 3_000_000_000, size=n).astype(U64)
    return k, T0 + sec, v, K


@pytest.mark.parametrize("T,n,sparse", [(4096, 30000, True), (4095, 30000, False), (4096, (1 << 21) - 1, True), (4096, 1 << 21, False)])
def test_sparse_rule(engine, T, n, sparse):
    """tad_capi_job.cpp (choose_stage0): sparse iff cells >= 2^24 && slots < cells / 8 — no plan override, the engine decides"""
    k, t, v, K = rule_table(T, n)
    cells = K * T
    assert lattice(t)[1:] == (1, T)
    assert sparse == (cells >= SPARSE_MIN_CELLS and n < cells // SPARSE_FILL)
    if n > 30000:
        assert abs(n - cells // SPARSE_FILL) <= 1 and cells == SPARSE_MIN_CELLS
    else:
        assert abs(cells - SPARSE_MIN_CELLS) <= K and n < (cells - K) // SPARSE_FILL
    paths = (4,) if sparse else DENSE_PATHS
    res, _ = check_lsd(engine, "EWMA", k, t, v, K, "svc", paths=paths)
    assert res.stats["n_buckets"] == T and res.stats["step"] == 1
    if n <= 30000:
        agg_check(engine, k, t, v, K, "svc", (4, 7) if sparse else DENSE_PATHS)
