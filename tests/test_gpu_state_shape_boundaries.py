"""GPU: the streaming-state kernels at every segment length, per-batch point count and total point count where they pick another code
path, bit for bit against references that do not share code with them (DESIGN.md §4 has the table):
  * k_hist_sort_wave / k_hist_sort_long: a key's new points of one batch sort in registers (b <= 64), by bitonic_flip in LDS (b <= 4096)
    or in place in global memory; k_hist_sort_long strides over its list beyond 2048 listed keys
  * k_hist_merge: one wavefront per 2048 elements of [old | new], old first on ties
  * k_trim_keep / k_trim_copy / k_hist_subtract / k_win_bounds / k_win_gather: chunks of 2048, chunk_key_min1's shortcut coff[K] == K
  * k_trim_moments / k_win_ewma / k_win_emit_staged: a lane walks its segment in chunks of 8, loaded two ahead
  * win_coop_min / k_win_route / k_win_ewma_coop: a wavefront per key from 512 points on, with K <= 8192 or len >= 8 (P / K + 1)
  * scan_launches: two launches up to 4096 * 2048 elements, three beyond

References: np.sort for a history, oracle/stream_oracle.py for moments, orc.run_job for rows, closed forms for the scan case (there the
stddev column alone comes from the engine's own tad_run on the same rows: "R1" of tests/test_gpu_state_run.py).  Float columns are
compared as uint64 bit patterns.  Every case asserts from host-side numbers (orc.stage0 of the batch, export_series(), win_coop_min
recomputed) that it sits on the edge it is named for before the engine is asked.  The helpers follow the neighbouring files (copied,
not imported).  The builders are plain functions of seeded numpy, usable without a GPU."""
import functools

import numpy as np
import pytest

from oracle import stream_oracle as so
from oracle import tad_oracle as orc
from state_helpers import COOP_MIN_T, HIST_CHUNK, STATE_FIELDS, T_BASE, U64, assert_rows, assert_same, bits, in_window, new_state, rows_of, snapshot

pytestmark = pytest.mark.gpu

# the constants of the kernels, mirrored (a change there must be followed here)
SORT_WAVE = 64                # tad_history.hip:48   k_hist_sort_wave: `if (b > 64)` lists the key for k_hist_sort_long
HIST_LDS = 4096               # tad_history.hip:25   kHistLdsPoints
SORT_LONG_GRID = 2048         # tad_history.hip:251  launch_hist_sort: min(K, 2048) workgroups of k_hist_sort_long
WALK_CHUNK = 8                # tad_history.hip:400  kTrimChunk; tad_window.hip:32 kWinChunk
COOP_MAX_K = 8192             # tad_internal.h:184   kCoopMaxK
SCAN_OWN_BASE = 4096 * 2048   # tad_kernels.hip:527  kScanOwnBaseBlocks x tad_kernels.hip:468 kScanTile

EPS = 1 << 24                 # the DBSCAN eps of the crafted cases: an integer, every distance below 2^53 is exact
ALPHA = 0.3                   # (the default 0.5 cannot see a wrong recurrence)


def clone(engine, K, snap):
    st = new_state(engine, K)
    st.load(snap["state"])
    st.load_history(*snap["history"])
    st.load_series(*snap["series"])
    if snap["times"] is not None:
        st.load_times(snap["times"])
    return st


def table(per_key, seed):
    """per_key: (key, second offsets, values) of every key's points -> the three columns, one row per point, rows in a seeded order"""
    k = np.concatenate([np.full(len(t), key, dtype=np.int64) for key, t, _ in per_key]).astype(U64)
    t = T_BASE + np.concatenate([np.asarray(t, dtype=np.int64) for _, t, _ in per_key])
    v = np.concatenate([np.asarray(x, dtype=np.int64) for _, _, x in per_key]).astype(U64)
    o = np.random.default_rng(seed).permutation(k.size)
    return np.ascontiguousarray(k[o]), np.ascontiguousarray(t[o]), np.ascontiguousarray(v[o])


def key_counts(k, t, v, K):
    """points per key of a batch, from the oracle's Stage 0"""
    pk, _, _ = orc.stage0(k, t, v, "max")
    return np.bincount(pk.astype(np.int64), minlength=K)


def sorted_per_key(pk, pv):
    """np.sort of every key's values, keys in order ((key, time)-ordered points in)"""
    return pv[np.lexsort((pv, pk))]


def rows_from(want, emit_all, sel=None):
    """the rows the engine must return, from orc.run_job's result; sel: a mask over the job's points"""
    pk, pt, pv = want["points"]
    m = np.ones(pk.size, bool) if sel is None else sel.copy()
    if not emit_all:
        m &= want["anomaly_all"]
    sig = np.repeat(want["sigma"], np.diff(want["ptr"]))
    d = {"key_id": pk[m], "flow_end_s": pt[m], "throughput": orc.u64_to_f64(pv)[m], "algo_calc": want["calc_all"][m], "stddev": sig[m]}
    if emit_all:
        d["anomaly"] = want["anomaly_all"][m].astype(np.uint8)
    return d


def oracle_moments(K, batches, alpha):
    """oracle/stream_oracle.py over the batches: the moments a state must hold"""
    ref = so.StreamState(K)
    for k, t, v in batches:
        if k.size:
            so.run_stream(ref, k, t, v, op="max", alpha=alpha)
    return ref


def assert_moments(st, ref, what=""):
    got = st.export()
    for f in STATE_FIELDS:
        assert np.array_equal(bits(got[f]), bits(np.ascontiguousarray(getattr(ref, f)).astype(got[f].dtype))), (what, f)


def both_verdicts_on_every_key(want, min_points=4):
    n = np.diff(want["ptr"])
    noisy = np.add.reduceat(want["anomaly_all"].astype(np.int64), want["ptr"][:-1])
    big = n >= min_points
    return bool(((noisy[big] > 0) & (noisy[big] < n[big])).all()) and bool((noisy[~big] == n[~big]).all())


# ------------------------------------------------------------------ 1: sorting one batch's new points
SORT_B = (1, 2, 63, 64, 65, 66, 96, 127, 128, 129, 255, 257, 1000, 2047, 2048, 2049, 4095, 4096, 4097, 5000, 8191, 8192, 8193)
FAMILIES = ("random40", "descending", "five")


def family_values(fam, n, rng):
    """n values in time order.  random40: a dense band (every point core at EPS) and n // 16 + 1 isolated points above it, below 2^40;
    descending: a chain EPS / 4 apart that falls with time, its first three points 3 EPS apart (noise); five: a set of five numbers,
    one of them on exactly two points (noise), the others many times (core) — ties everywhere.  Fewer than 4 points: all noise."""
    if fam == "random40":
        band = max(n * EPS // 8, 8)
        x = rng.integers(0, band, size=n)
        m = n // 16 + 1 if n >= 4 else 0
        x[:m] = band + 3 * EPS * (1 + np.arange(m)) + rng.integers(0, EPS // 2, size=m)
        x = x[rng.permutation(n)]
        assert x.max() < 1 << 40
    elif fam == "descending":
        x = 1_000_000_000 + (n - 1 - np.arange(n, dtype=np.int64)) * (EPS // 4)
        m = min(3, n - 1)
        x[:m] += 3 * EPS * (m - np.arange(m))
        assert (np.diff(x) < 0).all()
    else:
        s = 5_000_000_000 + EPS * np.array([0, 10, 20, 30, 40], dtype=np.int64)
        x = s[rng.integers(0, 4, size=n)]
        if n >= 6:
            x[rng.choice(n, size=2, replace=False)] = s[4]
    return x.astype(np.int64)


@functools.lru_cache(maxsize=None)
def sort_table():
    """one batch: a key for every (length, family), key order shuffled behind four fixed keys of 1, 64, 65 and 2 points (one workgroup
    of k_hist_sort_wave: a register sort beside a listed key beside keys that leave most lanes idle)"""
    rng = np.random.default_rng(64)
    combos = [(b, f) for b in SORT_B for f in FAMILIES]
    head = [(1, "random40"), (64, "random40"), (65, "random40"), (2, "five")]
    rest = [c for c in combos if c not in head]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    combos = head + rest
    per_key = [(i, np.arange(b), family_values(f, b, rng)) for i, (b, f) in enumerate(combos)]
    k, t, v = table(per_key, seed=65)
    return k, t, v, len(combos), np.array([b for b, _ in combos]), [f for _, f in combos]


@functools.lru_cache(maxsize=None)
def sort_oracle(which):
    k, t, v = (sort_table() if which == "edges" else stride_table())[:3]
    return orc.run_job("DBSCAN", k, t, v, op="max", eps=float(EPS), dbscan_fn=orc.dbscan_noise_sorted)


def check_sorted_batch(engine, tab, want, what):
    """one DBSCAN batch with emit_all on a fresh state: history = np.sort per key, rows = the oracle's"""
    k, t, v, K, lens = tab[:5]
    assert np.array_equal(key_counts(k, t, v, K), lens)                         # every key sits on its length
    pk, pt, pv = want["points"]
    assert both_verdicts_on_every_key(want)
    st = new_state(engine, K)
    got = engine.run_stream(st, k, t, v, agg_flow="", value_op="max", algo="DBSCAN", eps=float(EPS), emit_all=True)
    ln, vals = st.export_history()
    assert np.array_equal(ln, lens.astype(U64)), what
    assert np.array_equal(vals, sorted_per_key(pk, pv)), what
    assert np.array_equal(st.export_series()[1], pv) and np.array_equal(st.export_times(), pt), what
    assert_rows(rows_of(got), rows_from(want, True), what)
    st.close()
    return got


@pytest.mark.parametrize("plan,paths", [({"sparse": "always"}, (4, 8)), ({"sparse": "never"}, (1, 2, 3))], ids=["sparse", "dense"])
def test_history_sort_at_every_batch_length_edge(engine, plan, paths):
    """k_hist_sort_wave's register sort up to 64 points, bitonic_flip in LDS up to 4096 and in global memory beyond, at both ends of
    each range and at n just above and below a power of two; values random, already descending, and from a set of five"""
    tab = sort_table()
    lens, fams = tab[4], tab[5]
    assert lens[:4].tolist() == [1, 64, 65, 2]                                  # one workgroup of k_hist_sort_wave (four wavefronts)
    assert {(int(b), f) for b, f in zip(lens, fams)} == {(b, f) for b in SORT_B for f in FAMILIES}
    for edge in (SORT_WAVE, HIST_LDS):
        assert {edge - 1, edge, edge + 1} <= set(SORT_B)
    with engine.plan(**plan):
        got = check_sorted_batch(engine, tab, sort_oracle("edges"), plan)
    assert got.stats["stage0_path"] in paths, got.stats["stage0_path"]


@functools.lru_cache(maxsize=None)
def stride_table():
    """2300 keys on k_hist_sort_long's list: 100 of 4097 points (global memory), 100 of 300 and 2100 of 65 (LDS), interleaved"""
    rng = np.random.default_rng(2300)
    lens = np.array([4097 if i % 23 == 0 else 300 if i % 23 == 1 else 65 for i in range(2300)])
    per_key = [(i, np.arange(b), family_values("random40", int(b), rng)) for i, b in enumerate(lens)]
    k, t, v = table(per_key, seed=2301)
    return k, t, v, lens.size, lens


def test_history_sort_strides_over_more_listed_keys_than_workgroups(engine):
    """more listed keys than k_hist_sort_long has workgroups: a workgroup sorts an entry in LDS and then one in global memory, or the
    reverse, whatever order the atomics gave the list — s_v and the barrier after each entry are used twice"""
    tab = stride_table()
    lens = tab[4]
    assert ((lens == 65).sum(), (lens == 4097).sum(), (lens == 300).sum()) == (2100, 100, 100)
    assert (lens > SORT_WAVE).sum() == 2300 > SORT_LONG_GRID and (lens > HIST_LDS).sum() == 100
    check_sorted_batch(engine, tab, sort_oracle("stride"), "stride")


# ------------------------------------------------------------------ 2: merging a batch into the history (append path)
MERGE_PAIRS = ((0, 2049), (2049, 0), (2047, 1), (2047, 2), (2048, 1), (1, 2048), (2048, 2048), (2049, 2047), (4095, 2), (4096, 1), (6000, 70))
MERGE_FAMILIES = ("ties", "below", "above")
BATCH2 = 10000               # second offset of the second batch


@functools.lru_cache(maxsize=None)
def merge_batches():
    """two batches; key 2 i + 1 holds (a, b) = (old, new) points of pair i, the even keys hold nothing.  ties: old and new from the same
    3 to 7 numbers 3 EPS apart (the smallest of them only on the first old and the last new point: noise); below / above: every new value
    below / above every old one"""
    rng = np.random.default_rng(2048)
    combos = [(a, b, f) for f in MERGE_FAMILIES for a, b in MERGE_PAIRS]
    old, new = [], []
    for i, (a, b, f) in enumerate(combos):
        key = 2 * i + 1
        if f == "ties":
            d = 3 + i % 5
            s = 2_000_000_000 + 3 * EPS * np.arange(d, dtype=np.int64)
            xa, xb = s[rng.integers(1, d, size=a)], s[rng.integers(1, d, size=b)]
            if a:
                xa[0] = s[0]
            if b:
                xb[b - 1] = s[0]
        else:
            xa = 3_000_000_000 + rng.integers(0, 8 * EPS, size=a)
            xb = 3_000_000_000 + (-20 * EPS if f == "below" else 28 * EPS) + rng.integers(0, 8 * EPS, size=b)
        old.append((key, np.arange(a), xa))
        new.append((key, BATCH2 + np.arange(b), xb))
    return table(old, seed=1), table(new, seed=2), 2 * len(combos) + 1, combos


def test_history_merge_with_ties_at_every_chunk_edge(engine):
    """k_hist_merge: old[i] -> i + lower_bound(new), new[j] -> j + upper_bound(old).  Only values that tie between old and new show a
    swapped or doubled bound; merged lengths 2048, 2049, 4096, 4097 and 6070, a = 2048 exactly, a = 0 and b = 0, empty keys beside
    every multi-chunk key"""
    b1, b2, K, combos = merge_batches()
    a_want = np.zeros(K, dtype=np.int64)
    b_want = np.zeros(K, dtype=np.int64)
    for i, (a, b, _) in enumerate(combos):
        a_want[2 * i + 1], b_want[2 * i + 1] = a, b
    assert np.array_equal(key_counts(*b1, K), a_want) and np.array_equal(key_counts(*b2, K), b_want)
    assert {(a, b) for a, b, _ in combos} == set(MERGE_PAIRS) and (a_want[::2] == 0).all() and (b_want[::2] == 0).all()
    cat = [np.concatenate(c) for c in zip(b1, b2)]
    want1 = orc.run_job("DBSCAN", *b1, op="max", eps=float(EPS), dbscan_fn=orc.dbscan_noise_sorted)
    want2 = orc.run_job("DBSCAN", *cat, op="max", eps=float(EPS), dbscan_fn=orc.dbscan_noise_sorted)
    pk, pt, pv = want2["points"]
    off = np.concatenate([[0], np.cumsum(a_want + b_want)])
    for i, (a, b, f) in enumerate(combos):                                      # the families are what they claim, from the points
        key = 2 * i + 1
        seg_v, seg_t = pv[off[key]:off[key + 1]], pt[off[key]:off[key + 1]]
        xo, xn = seg_v[seg_t < T_BASE + BATCH2], seg_v[seg_t >= T_BASE + BATCH2]
        assert (xo.size, xn.size) == (a, b)
        if f == "ties":
            assert 3 <= np.unique(seg_v).size <= 7
            if a and b:
                assert np.intersect1d(xo, xn).size >= 1
            if a > 1 and b > 1:
                assert np.intersect1d(xo, xn).size >= 2
            h = np.sort(seg_v)
            if a + b > HIST_CHUNK:
                assert h[HIST_CHUNK - 1] == h[HIST_CHUNK]                       # a run of equal values crosses the chunk edge
        elif a and b:
            assert xn.max() < xo.min() if f == "below" else xn.min() > xo.max()
    second = pt >= T_BASE + BATCH2
    assert 0 < want2["anomaly_all"][second].sum() < second.sum()

    st = new_state(engine, K)
    got1 = engine.run_stream(st, *b1, agg_flow="", value_op="max", algo="DBSCAN", eps=float(EPS), emit_all=True, alpha=ALPHA)
    assert np.array_equal(st.export_series()[0], a_want.astype(U64))            # the old segments, from the state
    assert_rows(rows_of(got1), rows_from(want1, True), "batch 1")
    got2 = engine.run_stream(st, *b2, agg_flow="", value_op="max", algo="DBSCAN", eps=float(EPS), emit_all=True, alpha=ALPHA)
    ln, vals = st.export_history()
    assert np.array_equal(ln, (a_want + b_want).astype(U64))
    assert np.array_equal(vals, sorted_per_key(pk, pv))
    sl, sv = st.export_series()
    assert np.array_equal(sl, ln) and np.array_equal(sv, pv) and np.array_equal(st.export_times(), pt)
    assert_moments(st, oracle_moments(K, (b1, b2), ALPHA), "after batch 2")
    assert_rows(rows_of(got2), rows_from(want2, True, second), "batch 2")
    st.close()
    st = new_state(engine, K)                                                   # the anomalies-only rows of the same two batches
    engine.run_stream(st, *b1, agg_flow="", value_op="max", algo="DBSCAN", eps=float(EPS))
    got2 = engine.run_stream(st, *b2, agg_flow="", value_op="max", algo="DBSCAN", eps=float(EPS))
    assert_rows(rows_of(got2), rows_from(want2, False, second), "batch 2, anomalies")
    st.close()


# ------------------------------------------------------------------ 3: trim and window at chunk edges, runs of equal values
CHUNK_LENS = (2047, 2048, 2049, 4096, 4097, 6145)
VAL_A, VAL_B, VAL_D = 1_000_000_000, 1_000_000_000 + EPS // 2, 1_000_000_000 - 9 * EPS
LAYOUTS = {"edges": (0, 2047, 5, 2048, 0, 2049, 5, 4096, 0, 4097, 5, 6145, 0),
           "one chunk each": (2047, 0, 2048, 5, 2048, 0, 5, 1),
           "one key of two chunks": (2047, 0, 2048, 5, 2049, 0, 5, 1)}
BALLAST = 70000              # points of the extra key of the "ballast" state, all before T_BASE


def chunk_values(n, rng):
    """n values in time order from {A, B}, B on seven points of ten: in the sorted history B's run covers elements 2047 and 2048 of
    every key longer than a chunk.  The first and the last point are B; D, EPS away from everything, sits on two points (noise)."""
    x = np.where(rng.random(n) < 0.3, VAL_A, VAL_B).astype(np.int64)
    if n:
        x[0] = x[n - 1] = VAL_B
    if n >= 5:
        x[1] = x[n - 2] = VAL_D
    return x


@functools.lru_cache(maxsize=None)
def chunk_table(layout, ballast=False):
    rng = np.random.default_rng(len(layout))
    lens = list(LAYOUTS[layout])
    per_key = [(i, np.arange(n), chunk_values(n, rng)) for i, n in enumerate(lens)]
    if ballast:
        per_key.append((len(lens), np.arange(BALLAST) - BALLAST - 10000, chunk_values(BALLAST, rng)))
        lens.append(BALLAST)
    return table(per_key, seed=7) + (len(lens), np.array(lens))


def chunk_state(engine, layout, ballast=False):
    """the state of a layout after one EWMA batch, checked against the host's numbers: (state, (key, time, value) of its points)"""
    k, t, v, K, lens = chunk_table(layout, ballast)
    st = new_state(engine, K)
    engine.run_stream(st, k, t, v, agg_flow="", value_op="max", alpha=ALPHA)
    ln, vals = st.export_series()
    assert np.array_equal(ln, lens.astype(U64))                                 # the segment lengths, from the state
    W = (np.repeat(np.arange(K, dtype=U64), lens), st.export_times(), vals)
    pk, pt, pv = orc.stage0(k, t, v, "max")
    assert np.array_equal(W[0], pk) and np.array_equal(W[1], pt) and np.array_equal(W[2], pv)
    hv = st.export_history()[1]
    off = np.concatenate([[0], np.cumsum(lens)])
    for key in np.flatnonzero((lens > HIST_CHUNK) & (lens < BALLAST)):          # B's run straddles element 2048 of the history
        h = hv[off[key]:off[key + 1]]
        s = vals[off[key]:off[key + 1]]
        assert h[HIST_CHUNK - 1] == h[HIST_CHUNK] == VAL_B == s[0] == s[-1] and (s == VAL_B).sum() > 2
    return st, W


def trim_chunks(lens):
    """sum of k_trim_keep's / k_win_bounds' chunk counts: coff[K]"""
    lens = np.asarray(lens, dtype=np.int64)
    return int(np.where(lens > HIST_CHUNK, (lens + HIST_CHUNK - 1) // HIST_CHUNK, 1).sum())


def retained_mask(W, lens, keep_points=0, keep_from=0):
    """the points a trim keeps ((key, time)-ordered W): the time rule, then the newest keep_points"""
    k, t, _ = W
    m = t >= keep_from if keep_from else np.ones(k.size, bool)
    if keep_points:
        idx = np.flatnonzero(m)
        kk = k[idx]
        from_end = np.searchsorted(kk, kk, side="right") - np.arange(kk.size)
        m[idx[from_end > keep_points]] = False
    return m


def check_trim(engine, K, snap, W, lens, keep_points=0, keep_from=0):
    """a trim of a copy of the state: equal to a fresh state streamed the retained points, its history np.sort of them, its moments
    the streaming oracle's.  Returns the evicted count of every key."""
    m = retained_mask(W, lens, keep_points, keep_from)
    pts = tuple(np.ascontiguousarray(c[m]) for c in W)
    kept = np.bincount(pts[0].astype(np.int64), minlength=K)
    st = clone(engine, K, snap)
    dropped = st.trim(keep_points=keep_points, keep_from=keep_from, alpha=ALPHA)
    what = (keep_points, keep_from)
    assert dropped == W[0].size - pts[0].size, what
    ref = new_state(engine, K)
    if pts[0].size:
        engine.run_stream(ref, *pts, agg_flow="", value_op="max", alpha=ALPHA)
    got = snapshot(st)
    assert_same(got, snapshot(ref), what)
    assert np.array_equal(got["history"][0], kept.astype(U64)) and np.array_equal(got["history"][1], sorted_per_key(pts[0], pts[2])), what
    assert np.array_equal(got["series"][1], pts[2]), what
    assert_moments(st, oracle_moments(K, (pts,), ALPHA), what)
    ref.close()
    st.close()
    return lens - kept


def test_trim_cuts_at_every_chunk_edge(engine):
    """k_trim_keep / k_trim_copy / k_hist_subtract / k_trim_moments with the cut at element 1, 2047, 2048, 2049, len - 1 and len of keys
    of 2047 to 6145 points, by count and by time; the evicted prefix takes 1 copy and all but 1 copy out of the run of equal history
    values that crosses element 2048.  (keep_points = 0 means no count rule, so e = len is reached by time only.)"""
    K, lens = chunk_table("edges")[3:]
    assert sorted(set(lens.tolist()) - {0, 5}) == list(CHUNK_LENS) and trim_chunks(lens) > K
    st, W = chunk_state(engine, "edges")
    snap = snapshot(st)
    st.close()
    need = {(L, e) for L in CHUNK_LENS for e in (1, 2047, 2048, 2049, L - 1, L) if 0 < e <= L}
    by_count, by_time = set(), set()
    for kp in sorted({L - e for L, e in need if e < L}):
        ev = check_trim(engine, K, snap, W, lens, keep_points=kp)
        assert np.array_equal(ev, np.maximum(lens - kp, 0))
        by_count |= {(int(L), int(e)) for L, e in zip(lens, ev)}
    for e in sorted({e for _, e in need}):
        ev = check_trim(engine, K, snap, W, lens, keep_from=T_BASE + e)
        assert np.array_equal(ev, np.minimum(lens, e))
        by_time |= {(int(L), int(x)) for L, x in zip(lens, ev)}
    assert {p for p in need if p[1] < p[0]} <= by_count and need <= by_time
    # c = 1 of m > 2 (e = 1: the first point is B) and c = m - 1 (e = len - 1: the last point is B) on the run across element 2048:
    # chunk_state asserted first == last == B == history[2047] == history[2048] and more than two B on every key beyond a chunk
    assert {(L, 1) for L in CHUNK_LENS} | {(L, L - 1) for L in CHUNK_LENS} <= by_count & by_time


@pytest.mark.parametrize("layout", ["one chunk each", "one key of two chunks"])
def test_trim_with_and_without_the_one_chunk_shortcut(engine, layout):
    """chunk_key_min1 takes wavefront w for key w when coff[K] == K: every key at most 2048 points, empty keys included — and searches
    when exactly one key has 2049"""
    K, lens = chunk_table(layout)[3:]
    assert (trim_chunks(lens) == K) == (layout == "one chunk each") and lens.max() == (2048 if layout == "one chunk each" else 2049)
    assert (lens > HIST_CHUNK).sum() == (0 if layout == "one chunk each" else 1) and (lens == 0).sum() == 2
    st, W = chunk_state(engine, layout)
    snap = snapshot(st)
    st.close()
    for kp in (1, 2047, 2048):
        check_trim(engine, K, snap, W, lens, keep_points=kp)
    for e in (1, 5, 2047, 2048, 2049):
        check_trim(engine, K, snap, W, lens, keep_from=T_BASE + e)


# windows as (name, first element, element behind the last, keep_points): element j of every key is its point at T_BASE + j
WINDOWS = [("first to 2048th, exclusive", 0, 2047, 0), ("2048th and 2049th", 2047, 2049, 0), ("element 2047", 2047, 2048, 0),
           ("element 2048", 2048, 2049, 0), ("inside the second chunk", 2100, 3000, 0), ("empty", 7000, 7100, 0),
           ("everything", 0, 7000, 0), ("newest 1", 0, 7000, 1), ("newest 2048", 0, 7000, 2048), ("newest 2049", 0, 7000, 2049)] + \
          [("last element of %d" % L, L - 1, L, 0) for L in CHUNK_LENS if L not in (2048, 2049)]


def test_window_ranges_at_every_chunk_edge(engine):
    """k_win_bounds / k_win_gather / k_hist_subtract<true> / the window moments with the interior range beginning, ending and lying
    wholly inside any chunk.  The window's history is sorted from the window when 2 * window points <= state points and subtracted
    from the state's history otherwise: the wide windows go one way on the plain state and the other way on the same keys beside a
    key of 70000 older points; a narrow window cannot be made to subtract (it would have to hold more than half of the state)."""
    memo = {}
    ways = {}
    anomalies = {"EWMA": 0, "DBSCAN": 0}
    for ballast in (False, True):
        K, lens = chunk_table("edges", ballast)[3:]
        st, W = chunk_state(engine, "edges", ballast)
        S = W[0].size
        snap = snapshot(st)
        wins = WINDOWS + ([] if ballast else [("the whole state", None, None, 0)])
        for name, lo, hi, keep in wins:
            m = np.ones(S, bool) if lo is None else in_window(W[0], W[1], T_BASE + lo, T_BASE + hi, keep)
            Pw = int(m.sum())
            args = (0, 0, 0) if lo is None else (T_BASE + lo, T_BASE + hi, keep)
            by_sort = 2 * Pw <= S
            assert bool(engine._lib.tad_window_history_by_sort(Pw, S)) == by_sort, (name, Pw, S)
            ways.setdefault(name, set()).add(by_sort)
            cnt = np.bincount(W[0][m].astype(np.int64), minlength=K)
            if name == "element 2048":
                assert cnt.tolist()[:13] == [int(L > 2048) for L in lens[:13]] and Pw == 4
            if name == "inside the second chunk":
                assert set(cnt[:13].tolist()) == {0, 900} and (cnt[:13] == 900).sum() == 3
            if name == "empty":
                assert Pw == 0
            if name.startswith("newest"):
                assert np.array_equal(cnt[:13], np.minimum(lens[:13], keep))
            for algo in ("EWMA", "DBSCAN"):
                kw = dict(alpha=ALPHA) if algo == "EWMA" else dict(eps=float(EPS))
                if Pw and (name, algo) not in memo:
                    okw = dict(kw, dbscan_fn=orc.dbscan_noise_sorted) if algo == "DBSCAN" else kw
                    memo[name, algo] = orc.run_job(algo, W[0][m], W[1][m], W[2][m], op="max", **okw)
                for emit_all in (False, True):
                    got = engine.run_state_window(st, *args, algo=algo, emit_all=emit_all, **kw)
                    what = (name, ballast, algo, emit_all)
                    assert got.stats["n_points"] == Pw, what
                    if Pw == 0:
                        assert got.n_rows == 0, what
                    else:
                        assert_rows(rows_of(got), rows_from(memo[name, algo], emit_all), what)
                        anomalies[algo] += got.n_rows if not emit_all else 0
                assert_same(snapshot(st), snap, (name, ballast, algo, "state changed"))
        st.close()
    for name in ("first to 2048th, exclusive", "everything", "newest 2048", "newest 2049"):
        assert ways[name] == {True, False}, (name, ways[name])                  # built both ways
    assert ways["the whole state"] == {False} and ways["element 2047"] == {True}
    assert min(anomalies.values()) > 0, anomalies


# ------------------------------------------------------------------ 4: the lane walk in chunks of eight
LANE_LENS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40)


def lane_table(lens, seed):
    rng = np.random.default_rng(seed)
    per_key = []
    for i, n in enumerate(lens):
        base = 1_000_000_000 + int(orc.mix64(np.array([i + 5], dtype=U64))[0] % U64(3_000_000_000))
        per_key.append((i, np.sort(rng.choice(3600, size=n, replace=False)), base + rng.integers(-300_000_000, 300_000_000, size=n)))
    return table(per_key, seed + 1)


def test_lane_walk_at_every_prefetch_tail(engine):
    """k_win_ewma, k_win_emit_staged and k_trim_moments load two chunks of 8 ahead and consume the second only `if (c + 1 < nch)`:
    one chunk, a full and a started second, third, fourth and fifth one, with the last chunk holding 1, 7 and 8 points"""
    K = 200
    lens = np.array([LANE_LENS[i % len(LANE_LENS)] for i in range(K)])
    nch = (lens + WALK_CHUNK - 1) // WALK_CHUNK
    assert set(nch.tolist()) == {1, 2, 3, 4, 5} and {int(n % WALK_CHUNK) for n in LANE_LENS} >= {0, 1, 7}
    k, t, v = lane_table(lens, seed=8)
    assert np.array_equal(key_counts(k, t, v, K), lens)
    want = orc.run_job("EWMA", k, t, v, op="max", alpha=ALPHA)
    noisy = np.add.reduceat(want["anomaly_all"].astype(np.int64), want["ptr"][:-1])
    assert set(lens[noisy > 0].tolist()) == set(LANE_LENS) - {1} and want["n_anomalies"] > 64 * (K // 64)
    st = new_state(engine, K)
    engine.run_stream(st, k, t, v, agg_flow="", value_op="max", alpha=ALPHA)
    assert np.array_equal(st.export_series()[0], lens.astype(U64)) and lens.max() < COOP_MIN_T
    assert_rows(rows_of(engine.run_state(st, alpha=ALPHA)), rows_from(want, False), "count + staged emit")
    with engine.plan(ewma_emit_rows=64):
        assert_rows(rows_of(engine.run_state(st, alpha=ALPHA)), rows_from(want, False), "staged, 64 rows")
    with engine.plan(ewma_emit="lane"):
        assert_rows(rows_of(engine.run_state(st, alpha=ALPHA)), rows_from(want, False), "lane")
    assert_rows(rows_of(engine.run_state(st, alpha=ALPHA, emit_all=True)), rows_from(want, True), "emit_all")
    st.close()

    # the same lengths as what a trim and a window retain of 45 points per key
    full = np.full(K, 45)
    k, t, v = lane_table(full, seed=45)
    st = new_state(engine, K)
    engine.run_stream(st, k, t, v, agg_flow="", value_op="max", alpha=ALPHA)
    assert np.array_equal(st.export_series()[0], full.astype(U64))
    W = (np.repeat(np.arange(K, dtype=U64), full), st.export_times(), st.export_series()[1])
    snap = snapshot(st)
    for r in LANE_LENS:
        m = retained_mask(W, full, keep_points=r)
        pts = tuple(np.ascontiguousarray(c[m]) for c in W)
        assert (np.bincount(pts[0].astype(np.int64), minlength=K) == r).all() and r < 45            # every key: r retained, 45 - r evicted
        cp = clone(engine, K, snap)
        assert cp.trim(keep_points=r, alpha=ALPHA) == K * (45 - r)
        assert_moments(cp, oracle_moments(K, (pts,), ALPHA), ("trim", r))
        cp.close()
        ww = orc.run_job("EWMA", *pts, op="max", alpha=ALPHA)
        for emit_all in (True, False):
            got = engine.run_state_window(st, keep_points=r, alpha=ALPHA, emit_all=emit_all)
            assert_rows(rows_of(got), rows_from(ww, emit_all), ("window", r, emit_all))
        if r >= 2:
            assert ww["n_anomalies"] > 0
    assert_same(snapshot(st), snap, "state changed")
    st.close()


# ------------------------------------------------------------------ 5: a wavefront per key or a lane
COOP_LENS = (511, 512, 513, 575, 576, 577, 1024, 1025)


def coop_min(K, P):
    """win_coop_min (tad_window.hip:354), recomputed"""
    return COOP_MIN_T if K <= COOP_MAX_K else max(COOP_MIN_T, 8 * (P // K + 1))


def series_values(n, key, rng):
    base = 1_000_000_000 + int(orc.mix64(np.array([key + 5], dtype=U64))[0] % U64(3_000_000_000))
    return base + rng.integers(-300_000_000, 300_000_000, size=n)


def check_coop(engine, K, lens_by_key, fill, what, long_in_range=None):
    """a state of K keys: lens_by_key's lengths, every other key `fill` points (0 = unseen); EWMA at alpha 0.3 with and without
    emit_all against the oracle.  Returns the rule's threshold."""
    rng = np.random.default_rng(K + fill)
    lens = np.full(K, fill)
    for key, n in lens_by_key.items():
        lens[key] = n
    per_key = [(i, np.arange(n), series_values(int(n), i, rng)) for i, n in enumerate(lens) if n]
    k, t, v = table(per_key, seed=K)
    want = orc.run_job("EWMA", k, t, v, op="max", alpha=ALPHA)
    st = new_state(engine, K)
    engine.run_stream(st, k, t, v, agg_flow="", value_op="max", alpha=ALPHA)
    ln = st.export_series()[0].astype(np.int64)
    assert np.array_equal(ln, lens), what
    P = int(ln.sum())
    cm = coop_min(K, P)
    noisy = np.zeros(K, dtype=np.int64)
    noisy[want["keys"].astype(np.int64)] = np.add.reduceat(want["anomaly_all"].astype(np.int64), want["ptr"][:-1])
    for key, n in lens_by_key.items():
        assert noisy[key] > 0 or n < 2, (what, key)                             # rows on every key at an edge
    if long_in_range is not None:                                               # a wavefront's key inside a 64-key range of the staged emit:
        k0 = long_in_range // 64 * 64                                           # lanes' keys with rows before it and behind it
        lane = ln < cm
        assert ln[long_in_range] >= cm and noisy[long_in_range] > 0 and k0 < long_in_range < min(k0 + 63, K - 1)
        assert noisy[k0:long_in_range][lane[k0:long_in_range]].sum() > 0
        assert noisy[long_in_range + 1:k0 + 64][lane[long_in_range + 1:k0 + 64]].sum() > 0
    assert_rows(rows_of(engine.run_state(st, alpha=ALPHA)), rows_from(want, False), (what, "count + emit"))
    assert_rows(rows_of(engine.run_state(st, alpha=ALPHA, emit_all=True)), rows_from(want, True), (what, "emit_all"))
    with engine.plan(ewma_emit="lane"):
        assert_rows(rows_of(engine.run_state(st, alpha=ALPHA)), rows_from(want, False), (what, "lane emit"))
    st.close()
    return cm, ln


def test_window_walk_on_either_side_of_the_coop_rule(engine):
    """k_win_route lists a key for k_win_ewma_coop from win_coop_min points on: 512 with K <= 8192, max(512, 8 (P / K + 1)) beyond.
    Lengths on either side of 512, a multiple of 64 and one more (the last block of the walk is short), the same rows at K = 8192
    and 8193, and at K = 8193 with 64 points on every other key, where the threshold is 520"""
    for half in (COOP_LENS[:4], COOP_LENS[4:]):                                 # K = 5: two states, a short key with rows in the middle
        lens = {0: half[0], 1: half[1], 3: half[2], 4: half[3], 2: 9}
        cm, ln = check_coop(engine, 5, lens, 0, ("K = 5", half), long_in_range=1 if half[0] == 511 else None)
        assert cm == COOP_MIN_T and sorted(ln[ln >= cm].tolist()) == sorted(n for n in half if n >= 512)
    spots = {100 + 37 * i: n for i, n in enumerate(COOP_LENS)}                  # the same rows at both K; the others hold one point or none
    for K in (COOP_MAX_K, COOP_MAX_K + 1):
        lens = dict(spots)
        lens.update({key: 0 for key in range(5000, 5100)})                      # (unseen keys)
        cm, ln = check_coop(engine, K, lens, 1, ("K = %d" % K, "thin"))
        assert cm == COOP_MIN_T and (ln >= cm).sum() == 7 and ln[100] == cm - 1 and ln[137] == cm
    K = COOP_MAX_K + 1                                                          # the outlier rule above 512: 64 points on every other key
    lens = dict(spots)
    cm = 8 * 65
    lens.update({500: cm - 1, 501: cm, 8192: 70})
    cm_got, ln = check_coop(engine, K, lens, 64, "K = 8193, 64 points a key", long_in_range=100 + 37 * 4)
    assert cm_got == cm == 520 and ln.sum() // K == 64
    assert sorted(ln[ln >= cm].tolist()) == [520, 575, 576, 577, 1024, 1025] and (ln == cm - 1).sum() == 1 and {511, 512, 513} <= set(ln.tolist())


# ------------------------------------------------------------------ 6: the scan over more than 4096 * 2048 elements
@functools.lru_cache(maxsize=2)
def scan_table(extra_key):
    """4096 keys x 2048 points (+ one key with one point): key k at base_k + (j mod 7); where mix64(2048 k + j) = 0 mod 257 the value
    is base_k + 4e9 + j 1e9: isolated at the default eps 2.5e8, and nothing else is (the one-point key is noise: fewer than 4 points)"""
    Kf, n = 4096, 2048
    kk = np.repeat(np.arange(Kf, dtype=np.int64), n)
    jj = np.tile(np.arange(n, dtype=np.int64), Kf)
    base = 1_000_000_000 + 1000 * kk
    planted = orc.mix64((kk * n + jj).astype(U64)) % U64(257) == 0
    val = np.where(planted, base + 4_000_000_000 + jj * 1_000_000_000, base + jj % 7)
    if extra_key:
        kk, jj = np.append(kk, Kf), np.append(jj, 0)
        val, planted = np.append(val, 1_000_000_000 + 1000 * Kf), np.append(planted, True)
    assert val.max() < 1 << 53
    return (np.ascontiguousarray(kk.astype(U64)), np.ascontiguousarray(T_BASE + jj), np.ascontiguousarray(val.astype(U64)),
            Kf + int(extra_key), planted)


@pytest.mark.parametrize("extra_key", [False, True], ids=["4096 blocks", "4097 blocks"])
def test_scan_over_points_on_either_side_of_4096_blocks(engine, extra_key):
    """launch_scan over the points of one batch (tad_run_stream DBSCAN) and of a state (tad_run_state DBSCAN): 4096 * 2048 elements
    take k_scan_apply<true>, one more takes k_scan_top and k_scan_apply<false>"""
    k, t, v, K, planted = scan_table(extra_key)
    P = k.size
    assert P == SCAN_OWN_BASE + int(extra_key) and (P + 2047) // 2048 == 4096 + int(extra_key)
    at = np.flatnonzero(planted)
    assert planted[:2048].any() and planted[255 * 2048:257 * 2048].any() and (at // 2048).max() == (P - 1) // 2048
    if extra_key:
        assert planted[P - 1] and at[-1] // 2048 == 4096                         # a row in the block behind the 4096th
    r1 = engine.run("DBSCAN", k, t, v, K, agg_flow="", value_op="max")          # R1: the stddev column
    assert r1.n_rows == at.size
    want = {"key_id": k[at], "flow_end_s": t[at], "throughput": v[at].astype(np.float64), "algo_calc": np.zeros(at.size),
            "stddev": np.asarray(r1["stddev"])}
    assert_rows(rows_of(r1), want, "tad_run")
    st = new_state(engine, K)
    got = engine.run_stream(st, k, t, v, agg_flow="", value_op="max", algo="DBSCAN")
    assert got.n_rows == at.size
    assert_rows(rows_of(got), want, "run_stream")
    assert st.series_points() == P == st.history_points()
    got = engine.run_state(st, algo="DBSCAN")
    assert got.n_rows == at.size and got.stats["n_points"] == P
    assert_rows(rows_of(got), want, "run_state")
    st.close()
