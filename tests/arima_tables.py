"""Tables for tests/test_gpu_arima_boundaries.py, and what the oracle says about them.  No engine call on this side:
tests/test_arima_tables.py checks on the host that every table is what its builder claims (series lengths, keys without a result,
per-position fit counts, few non-finite predictions), so that a green GPU comparison means something.

One row per point, so that Stage 0 changes nothing; a point's time is T0 + 60 * bucket.  Values: floor(3e6 * exp(N(0, 0.3))) + 1, the
middle point of a series of more than 4 points times 3 (the base of tests/test_gpu_arima.py:test_series_arima_every_length).  Every
builder is deterministic; the seeds are the ones at which the tables meet test_arima_tables.py's conditions.

The constants the tables sit on (theia_amd/csrc/tad_arima.hip): kStage = 8 (the staged rounds of the fit, Tpad = roundup8(T), the batches
of eight buckets of k_arima_prep), 64 keys per wavefront of k_arima_start, 256 keys per block of k_arima_prep, kArimaChunk = 4096 keys per
wavefront and position of k_arima_fit, and, for a streaming batch, 64 fits per wavefront and position (stream_arima_batch's chunk)."""
import time

import numpy as np

from oracle import tad_oracle as orc

T0 = orc.SYNTH_T_BASE
STEP = orc.SYNTH_T_STEP
U64 = np.uint64
NAN_CAP = 0.01            # share of NaN predictions a table may have (a condition on the inputs, never on the engine)
ORACLE_SECONDS = 5.0      # no table whose oracle run needs more


class Table:
    """rows (key, t, v) over K keys on a lattice of T buckets; lengths[k] = points of key k as built; no_result = the ids built without
    a result (<= 3 points, constant, or holding a zero) that have at least one point"""

    def __init__(self, name, key, t, v, K, T, lengths, no_result=()):
        self.name, self.K, self.T = name, int(K), int(T)
        self.key, self.t, self.v = np.asarray(key, U64), np.asarray(t, np.int64), np.asarray(v, U64)
        self.lengths = np.asarray(lengths, np.int64)
        self.no_result = tuple(sorted(int(k) for k in no_result))

    @property
    def rows(self):
        return self.key, self.t, self.v

    @property
    def lattice(self):
        return (T0, STEP, self.T)

    def with_result(self):
        m = self.lengths > 3
        m[list(self.no_result)] = False
        return m

    def expected_no_result(self):
        """keys with at least one point and no result: exact, from the builder alone"""
        short = (self.lengths > 0) & (self.lengths <= 3)
        return int(short.sum()) + sum(1 for k in self.no_result if self.lengths[k] > 3)

    def expected_fits(self):
        return int(np.clip(self.lengths - 3, 0, None)[self.with_result()].sum())

    def fits_per_position(self):
        """cnt[p] = keys with a result and more than p points, p >= 3 (the fits k_arima_fit runs at position p)"""
        n = self.lengths[self.with_result()]
        return np.array([0, 0, 0] + [int((n > p).sum()) for p in range(3, self.T)], np.int64)[:max(self.T, 3)]


_WANT = {}


def want(tab):
    """orc.run_job("ARIMA") on the table, computed once per process and shared (read-only) by every test that needs it; the oracle's
    time is kept in want["seconds"]"""
    if tab.name not in _WANT:
        t0 = time.perf_counter()
        w = orc.run_job("ARIMA", tab.key, tab.t, tab.v, agg_flow="svc")
        w["seconds"] = time.perf_counter() - t0
        _WANT[tab.name] = w
    return _WANT[tab.name]


def values(rng, n):
    v = np.floor(3e6 * np.exp(rng.normal(0.0, 0.3, n))).astype(U64) + U64(1)
    if n > 4:
        v[n // 2] *= U64(3)
    return v


def from_series(name, series, K, T, seed, no_result=()):
    """series: {key id: (buckets, values)} -> a Table with its rows shuffled"""
    rng = np.random.default_rng(seed)
    ids = sorted(series)
    key = np.concatenate([np.full(len(series[k][0]), k, U64) for k in ids] + [np.zeros(0, U64)])
    b = np.concatenate([np.asarray(series[k][0], np.int64) for k in ids] + [np.zeros(0, np.int64)])
    v = np.concatenate([np.asarray(series[k][1], U64) for k in ids] + [np.zeros(0, U64)])
    assert b.size == 0 or (0 <= b.min() and b.max() < T)
    o = rng.permutation(key.size)
    lengths = np.zeros(K, np.int64)
    for k in ids:
        assert len(set(series[k][0])) == len(series[k][0]) == len(series[k][1])
        lengths[k] = len(series[k][0])
    return Table(name, key[o], T0 + STEP * b[o], v[o], K, T, lengths, no_result)


def series_of(tab):
    """{key id: (buckets, values)} in time order"""
    o = np.lexsort((tab.t, tab.key))
    k, b, v = tab.key[o], (tab.t[o] - T0) // STEP, tab.v[o]
    keys, ptr = orc.series_offsets(k)
    return {int(kk): (b[a:z], v[a:z]) for kk, a, z in zip(keys, ptr[:-1], ptr[1:])}


# ---- ragged lengths ----
def ragged(K, T, seed, cap=None):
    """Key k has k % (top + 1) points, top = T (cap: top = cap, every series below full length: the positions from cap on have no fit
    and their wavefronts run dry on the first refill).  The first bucket varies from key to key.  Every other cycle of lengths has
    holes: the present buckets after the first are drawn at random, without repeats, from the buckets after the first; the other
    cycles are contiguous.  The first and the last bucket of the lattice are present (a full-length key, or, with a cap, the longest)."""
    rng = np.random.default_rng(seed)
    top = T if cap is None else int(cap)
    assert 4 <= top <= T
    series = {}
    for k in range(K):
        n = k % (top + 1)
        if n == 0:
            continue
        cycle = k // (top + 1)
        first = (k * 7 + cycle) % (T - n + 1)
        if cap is not None and n == top:
            first = (0, T - n)[cycle % 2]          # the longest keys alternately reach the first and the last bucket
        if cycle % 2 == 1 and n > 1:
            rest = np.sort(rng.choice(np.arange(first + 1, T), size=n - 1, replace=False))
            b = np.concatenate([[first], rest])
        else:
            b = first + np.arange(n)
        series[k] = (b, values(rng, n))
    name = "ragged(%d,%d,%d%s)" % (K, T, seed, "" if cap is None else ",cap=%d" % cap)
    return from_series(name, series, K, T, seed + 1)


def with_no_result_keys(tab, at):
    """The keys `at` replaced by, in turn, a constant series of 6 points, a series of 6 points holding a zero and a 3-point series
    (at must name key 0, lanes 63 and 64 and the last key: the first lane of k_arima_prep's first wavefront, the last lane of it, the
    first of the next, and the table's last lane, whose wavefront is partly beyond K)"""
    at = [int(a) for a in at]
    assert {0, 63, 64, tab.K - 1} <= set(at) or tab.K <= 64
    rng = np.random.default_rng(len(at) * 1000 + tab.K)
    series = series_of(tab)
    for i, k in enumerate(at):
        first = k % (tab.T - 6 + 1)
        kind = i % 3
        if kind == 0:
            series[k] = (first + np.arange(6), np.full(6, 9, U64))
        elif kind == 1:
            v = values(rng, 6)
            v[1 + i % 4] = 0
            series[k] = (first + np.arange(6), v)
        else:
            series[k] = (first + 2 * np.arange(3), values(rng, 3))
    return from_series(tab.name + "+noresult" + str(tuple(at)), series, tab.K, tab.T, 7, no_result=at)


def lane_edges(K):
    return sorted({0, 63, 64, K - 1})


# ---- seams inside a series ----
SEAM_CLASSES = 8


def seam_holes(K, T):
    """Key k by k % 8:
    0  every bucket;
    1  buckets [5, 11) only: 6 points that straddle the first eight-bucket seam;
    2  T % 8 != 0: only the buckets of k_arima_prep's tail loop, [T - T % 8, T) (T = 17: one point, T = 23: seven);
       T % 8 == 0: buckets [T - 11, T - 5), the straddle of the last seam;
    3  every bucket but 7, 8, 15 and 16;
    4  every bucket but 7;       5  every bucket but 8;       6  every bucket but 15 and 16;
    7  buckets [0, 8) only: the series ends with the first batch of eight."""
    assert T >= 16
    rng = np.random.default_rng(1000 * T + K)
    allb = np.arange(T)
    series = {}
    for k in range(K):
        c = k % SEAM_CLASSES
        if c == 0:
            b = allb
        elif c == 1:
            b = np.arange(5, 11)
        elif c == 2:
            b = np.arange(T - T % 8, T) if T % 8 else np.arange(T - 11, T - 5)
        elif c == 3:
            b = allb[~np.isin(allb, (7, 8, 15, 16))]
        elif c == 4:
            b = allb[allb != 7]
        elif c == 5:
            b = allb[allb != 8]
        elif c == 6:
            b = allb[~np.isin(allb, (15, 16))]
        else:
            b = np.arange(8)
        series[k] = (b, values(rng, b.size))
    return from_series("seam_holes(%d,%d)" % (K, T), series, K, T, 1000 * T + K + 1)


# ---- the grid T against 8, the key count against 64 / 256 / 4096: the synthetic table ----
def synth(K, T, rows_per_cell=2, drop_fifth=False, const_key0=False, seed=orc.SYNTH_SEED):
    """orc.synth_rows over K keys x T buckets; drop_fifth: a fifth of the cells removed — every key but each eighth (k % 8 == 0, which
    keeps all T buckets, so that the last position has fits) loses the rows of its cells with mix64(key * 4099 + bucket) % 9 < 2;
    const_key0: key 0's rows replaced by a constant series on every bucket (a key without a result in lane 0)"""
    k, t, v = orc.synth_rows(0, K * T * rows_per_cell, K, T, seed=seed)
    if drop_fifth:
        b = ((t - T0) // STEP).astype(U64)
        keep = (k % U64(8) == 0) | (orc.mix64(k * U64(4099) + b) % U64(9) >= 2)
        k, t, v = k[keep], t[keep], v[keep]
    if const_key0:
        keep = k != 0
        k = np.concatenate([k[keep], np.zeros(T, U64)])
        t = np.concatenate([t[keep], T0 + STEP * np.arange(T, dtype=np.int64)])
        v = np.concatenate([v[keep], np.full(T, 1_000_000, U64)])
    pk, _, _ = orc.stage0(k, t, v, "sum")
    lengths = np.bincount(pk.astype(np.int64), minlength=K)
    name = "synth(%d,%d,%d,%d,%d,%d)" % (K, T, rows_per_cell, drop_fifth, const_key0, seed - orc.SYNTH_SEED)
    return Table(name, k, t, v, K, T, lengths, no_result=(0,) if const_key0 and T > 3 else ())


# ---- the tables of the GPU file, by name (built on demand, once per process) ----
GRID_T = (3, 4, 7, 8, 9, 15, 16, 17, 25)
GRID_CASES = [(T, 70) for T in GRID_T] + [(15, 71), (17, 71), (25, 71)]          # odd K x odd T: the odd-cell carve
KEY_CASES = [(K, 17) for K in (1, 2, 63, 64, 65, 255, 256, 257)] + [(K, T) for T in (9, 17) for K in (4095, 4096, 4097)]
RAGGED_CASES = [(131, 41, 3, None), (259, 65, 5, None), (4097, 17, 9, None), (131, 41, 3, 39), (4097, 17, 9, 15)]
SEAM_CASES = [(67, 16), (67, 17), (67, 23)]
_TABLES = {}


def _cached(key, build):
    if key not in _TABLES:
        _TABLES[key] = build()
    return _TABLES[key]


# synth_rows' seed is SYNTH_SEED + the number here where the default's table misses a condition of test_arima_tables.py
GRID_SEEDS = {}
KEY_SEEDS = {(4096, 9): 1}        # (the default seed holds a key of 9 points whose Box-Cox bracket fails: a key without a result nobody built)


def grid_table(T, K, seed=None):
    seed = orc.SYNTH_SEED + (GRID_SEEDS.get((T, K), 0) if seed is None else seed)
    return _cached(("grid", T, K, seed), lambda: synth(K, T, rows_per_cell=12, drop_fifth=True, seed=seed))


def key_table(K, T, seed=None):
    seed = orc.SYNTH_SEED + (KEY_SEEDS.get((K, T), 0) if seed is None else seed)
    return _cached(("keys", K, T, seed), lambda: synth(K, T, const_key0=K == 2, seed=seed))


def ragged_table(K, T, seed, cap):
    return _cached(("ragged", K, T, seed, cap), lambda: with_no_result_keys(ragged(K, T, seed, cap), lane_edges(K)))


def seam_table(K, T):
    return _cached(("seam", K, T), lambda: seam_holes(K, T))


def all_tables():
    for T, K in GRID_CASES:
        yield grid_table(T, K)
    for K, T in KEY_CASES:
        yield key_table(K, T)
    for c in RAGGED_CASES:
        yield ragged_table(*c)
    for K, T in SEAM_CASES:
        yield seam_table(K, T)


# ---- stream batches ----
class StreamCase:
    """Two batches on K keys: batch 0 gives key k its old[k] points, batch 1 its new[k] points (touched keys: new > 0), every key on
    consecutive buckets from first[k] (default 0).  bad: keys without a result although they have more than 3 points, in turn constant
    from the start and holding a zero in their last point (which arrives with batch 1 when the key is touched)."""

    def __init__(self, name, K, old, new, bad=(), seed=0, first=None):
        rng = np.random.default_rng(seed)
        self.name, self.K = name, int(K)
        self.old, self.new = np.asarray(old, np.int64), np.asarray(new, np.int64)
        assert self.old.size == self.new.size == K
        self.first = np.zeros(K, np.int64) if first is None else np.asarray(first, np.int64)
        self.bad = tuple(int(k) for k in bad)
        self.constant = self.bad[0::2]
        n = self.old + self.new
        rows = [[], []]
        for k in range(K):
            if n[k] == 0:
                continue
            v = values(rng, int(n[k]))
            if k in self.constant:
                v[:] = 7
            elif k in self.bad:
                v[int(n[k]) - 1] = 0
            b = np.arange(n[k], dtype=np.int64)
            for h, sel in ((0, b < self.old[k]), (1, b >= self.old[k])):
                rows[h].append((np.full(int(sel.sum()), k, U64), T0 + STEP * (self.first[k] + b[sel]), v[sel]))
        self.batches = []
        for h in (0, 1):
            cat = [np.concatenate([r[i] for r in rows[h]] + [np.zeros(0, d)]) for i, d in enumerate((U64, np.int64, U64))]
            o = rng.permutation(cat[0].size)
            self.batches.append(tuple(c[o] for c in cat))

    def touched(self, batch=1):
        return np.flatnonzero((self.new if batch else self.old) > 0)

    def with_result(self, batch=1):
        """keys whose series after the batch has a result"""
        n = self.old + self.new if batch else self.old
        m = n > 3
        zero_in = [k for k in self.bad if k not in self.constant and (batch or self.new[k] == 0)]
        m[list(self.constant) + zero_in] = False
        return m

    def fits_per_position(self, batch=1):
        """cnt[p] of the batch's fit lists: touched keys with a result and max(old, 3) <= p < n (batch 0: nothing is old)"""
        lo = np.maximum(self.old if batch else 0, 3)
        hi = self.old + self.new if batch else self.old
        ok = self.with_result(batch)
        return np.array([int((ok & (lo <= p) & (p < hi)).sum()) for p in range(int(hi.max()))], np.int64)

    def expected_fits(self, batch=1):
        return int(self.fits_per_position(batch).sum())

    def expected_no_result(self, batch=1):
        t = np.zeros(self.K, bool)
        t[self.touched(batch)] = True
        return int((t & ~self.with_result(batch)).sum())

    def concat(self, upto):
        return tuple(np.concatenate([b[i] for b in self.batches[:upto + 1]]) for i in range(3))


def stream_fits_at(p_star, m, K=200, seed=0):
    """Batch 1 has exactly m fits at position p_star: m keys grow from p_star - 1 to p_star + 2 points; the other touched keys end at
    p_star points (fits below p_star only) or start at p_star + 1 (fits above it only).  Untouched keys lie between them."""
    assert p_star >= 4 and 3 * m // 2 + 20 < K
    old, new = np.zeros(K, np.int64), np.zeros(K, np.int64)
    ids = np.arange(K)
    hit = ids[ids % 3 != 2][:m]                                  # m keys, two of every three ids
    old[hit], new[hit] = p_star - 1, 3
    rest = ids[ids % 3 == 2]
    below, above, idle = rest[0::3], rest[1::3], rest[2::3]
    old[below], new[below] = p_star - 2, 2                       # n = p_star: positions < p_star
    old[above], new[above] = p_star + 1, 2                       # lo = p_star + 1
    old[idle] = 6                                                # untouched
    other = ids[ids % 3 != 2][m:]
    old[other] = 5                                               # untouched
    return StreamCase("fits_at(%d,%d)" % (p_star, m), K, old, new, seed=seed + m)


def stream_lengths(seed=3):
    """Series lengths after the batch n in {7, 8, 9, 15, 16, 17}, neighbouring slots back to back (every key touched: len8 = roundup8(n)
    is the only thing between two series in the packed ysk), old from 0 to n - 1 in turn"""
    ns = (7, 8, 9, 15, 16, 17)
    K = 72
    n = np.array([ns[k % 6] for k in range(K)], np.int64)
    old = np.array([(k // 6 * 3 + k) % n[k] for k in range(K)], np.int64)
    return StreamCase("lengths", K, old, n - old, seed=seed)


def stream_old_new(seed=2):
    """old in {0 .. 4} x new in {1 .. 4}: new points at p < 3, straddling 3, and from 3 on; three keys of each, an untouched key after
    every touched one"""
    combos = [(o, w) for o in range(5) for w in range(1, 5)] * 3
    K = 2 * len(combos)
    old, new = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for i, (o, w) in enumerate(combos):
        old[2 * i], new[2 * i] = o, w
        old[2 * i + 1] = 5 + i % 4
    return StreamCase("old_new", K, old, new, seed=seed)


def stream_touched(m, K=600, seed=3):
    """m touched keys of K, spread evenly with untouched keys between them; the touched keys at slot 0 (m > 1) and slot 63 (m > 63)
    have no result: one constant, one whose new points hold a zero"""
    old, new = np.zeros(K, np.int64), np.zeros(K, np.int64)
    ids = np.arange(K)
    old[:] = 4 + ids % 5
    touched = (np.arange(m) * K) // m
    assert np.unique(touched).size == m
    new[touched] = 1 + np.arange(m) % 4
    old[touched[::7]] = np.arange(touched[::7].size) % 4          # some touched keys are young: old in 0 .. 3
    bad = ([touched[0]] if m > 1 else []) + ([touched[63]] if m > 63 else [])
    for k in bad:
        old[k], new[k] = 4, 2
    return StreamCase("touched(%d)" % m, K, old, new, bad=bad, seed=seed + m)


def window_cut_state(seed=4):
    """every key with 12 points, key k on buckets k % 3 .. k % 3 + 11: a time range that ends before bucket 5, 6 or 10 cuts the series
    at 5 | 4 | 3, 6 | 5 | 4 and 10 | 9 | 8 points, one that starts at bucket 8 at 4 | 5 | 6"""
    K = 70
    old = np.full(K, 12, np.int64)
    return StreamCase("window", K, old, np.zeros(K, np.int64), seed=seed, first=np.arange(K) % 3)
