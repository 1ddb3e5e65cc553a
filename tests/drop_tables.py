"""Tables, a vectorised mirror of the oracle's pairwise sum and the expected rows for tests/test_gpu_drop_boundaries.py.  No engine call on
this side: tests/test_oracle_drop.py holds the mirror to oracle.drop_oracle.pairwise_sum and to numpy's add-reduce at every length used
here, and checks the tables' order-sensitivity condition on the host.

Values.  Counts of a few units add up exactly in any order and cannot tell one summation order from another.  Here a point's value is
uniform in [2^52, 2^53) — every addition of two of them rounds — and every second key has one value dipped to [2^40, 2^41), a point
far below mean - 3 std once the key has 11 points.  One row per point unless a table says otherwise, so that Stage 0 changes nothing.

The condition (assert_order_sensitive): for every length n >= 4 at least two keys of the table have a value sum AND a squared-deviation
sum that differ from the sum in the wrong order — left to right (np.cumsum) for n >= 8, the accumulator tree on the zero-padded series
((a0+a1)+(a2+a3))+((a4+a5)+(a6+0)) for 4 <= n < 8, the order a kernel would produce that took the accumulator branch too early.  n = 3 is
exempt: (a0+a1)+a2 both ways.  Keys are drawn by rejection on the host until they qualify."""
import numpy as np

from oracle import drop_oracle as dro
from oracle import tad_oracle as orc
from state_helpers import ROW_FIELDS, bits, pairwise_rows as pairwise_rows_8_to_128

DAY = 86400
T_BASE = 19000 * DAY
SHORT_LENGTHS = list(range(1, 301))
LONG_LENGTHS = list(range(511, 530)) + list(range(1023, 1042)) + [2049, 4100]
ALL_LENGTHS = SHORT_LENGTHS + LONG_LENGTHS
COUNTERS = ("n_keys", "n_points", "n_anomalies", "keys_no_result")


# ---- the oracle's sum, vectorised over rows ----
def pairwise_rows(A):
    """dro.pairwise_sum over every row of A, any number of columns: the same additions in the same order"""
    n = A.shape[1]
    if n < 8:
        r = np.zeros(A.shape[0])
        for i in range(n):
            r = r + A[:, i]
        return r
    if n <= 128:
        return pairwise_rows_8_to_128(A)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_rows(A[:, :n2]) + pairwise_rows(A[:, n2:])


def tree_of_eight_rows(A):
    """4 <= columns < 8: the accumulator branch's final tree over the zero-padded rows"""
    r = [A[:, j] if j < A.shape[1] else np.zeros(A.shape[0]) for j in range(8)]
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))


def wrong_order_rows(A):
    return np.cumsum(A, axis=1)[:, -1] if A.shape[1] >= 8 else tree_of_eight_rows(A)


def order_sensitive_rows(X):
    """per row of X (float64, >= 4 columns): both sums differ from the wrong order's"""
    n = X.shape[1]
    s = pairwise_rows(X)
    sq = (s[:, None] / n - X) ** 2
    return (s != wrong_order_rows(X)) & (pairwise_rows(sq) != wrong_order_rows(sq))


def order_sensitive(x, values_too=True):
    """the same for one series, from the oracle's own functions; values_too=False: the squared-deviation sum alone"""
    x = np.asarray(x, dtype=np.float64)
    wrong = (lambda a: float(np.cumsum(a)[-1])) if x.size >= 8 else (lambda a: float(tree_of_eight_rows(a[None, :])[0]))
    if values_too and dro.pairwise_sum(x) == wrong(x):
        return False
    sq = (dro.drop_stats(x)[0] - x) ** 2
    return dro.pairwise_sum(sq) != wrong(sq)


# ---- values ----
def draw(rng, shape, dip_rows=False):
    """uniform in [2^52, 2^53); dip_rows: one value of every row in [2^40, 2^41)"""
    v = rng.integers(1 << 52, 1 << 53, size=shape, dtype=np.uint64)
    if dip_rows and v.shape[1]:
        at = rng.integers(0, v.shape[1], size=v.shape[0])
        v[np.arange(v.shape[0]), at] = rng.integers(1 << 40, 1 << 41, size=v.shape[0], dtype=np.uint64)
    return v


def draw_key(rng, n, dip, batches=64):
    """a key of n points: the first of 32 draws that is order-sensitive, 32 more up to `batches` times (n < 4: the first draw)"""
    for _ in range(batches):
        C = draw(rng, (32, n), dip)
        if n < 4:
            return C[0]
        ok = np.flatnonzero(order_sensitive_rows(orc.u64_to_f64(C.ravel()).reshape(C.shape)))
        if ok.size:
            return C[ok[0]]
    return C[0]


def days_of(rng, n, scattered, first_day):
    """n day numbers in order: contiguous from day 0, or from first_day with one to three days to the next (at least two missing days
    somewhere once n >= 3)"""
    if not scattered:
        return np.arange(n, dtype=np.int64)
    gaps = rng.choice(np.array([1, 1, 1, 2, 3]), size=max(n - 1, 0))
    if n >= 3 and gaps.sum() < n + 1:
        gaps[rng.integers(0, n - 1)] = 3
    return first_day + np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)


class DropTable:
    """rows (key, t, v) over K keys, the Stage 0 arguments of the job, and — cached, read-only — what the oracle says about them"""

    def __init__(self, key, t, v, K, lengths=None, **stage0):
        self.key, self.t, self.v, self.K = key, t, v, int(K)
        self.lengths = lengths                      # per key id, when the builder knows them
        self.stage0 = stage0                        # value_op, key_id2, flow_start_s, start_time, end_time
        self._points = None
        self._want = {}

    def engine_kw(self):
        kw = dict(self.stage0)
        kw.setdefault("value_op", "sum")
        kw["agg_flow"] = "pod" if "key_id2" in kw else "svc"
        return kw

    def points(self):
        """(pk, pt, x, ptr, stats): Stage 0's points in (key, time) order, the series offsets, (mean, std) per key with >= 2 points"""
        if self._points is None:
            s0 = self.stage0
            pk, pt, pv = orc.stage0(self.key, self.t, self.v, s0.get("value_op", "sum"), s0.get("key_id2"), s0.get("flow_start_s"),
                                    s0.get("start_time", 0), s0.get("end_time", 0))
            keys, ptr = orc.series_offsets(pk)
            x = orc.u64_to_f64(pv)
            stats = np.array([dro.drop_stats(x[a:b]) if b - a >= 2 else (0.0, 0.0) for a, b in zip(ptr[:-1], ptr[1:])]).reshape(-1, 2)
            self.pv = pv                            # the points' integer values, for the series entry point
            self._points = (pk, pt, x, ptr, stats)
        return self._points

    def want(self, nsigma=3.0, ms=3):
        """(oracle.drop_oracle.run_job's result, the emit_all rows).  The emit_all rows are built from the per-key statistics; that their
        anomalous rows ARE run_job's rows is asserted here, so run_job stays the reference for both."""
        if (nsigma, ms) not in self._want:
            job = dro.run_job(self.key, self.t, self.v, n_sigma=nsigma, min_samples=ms, **self.stage0)
            pk, pt, x, ptr, stats = self.points()
            n = np.diff(ptr)
            kept = np.repeat((n >= ms) & (n >= 2), n)
            mean, std = np.repeat(stats[:, 0], n), np.repeat(stats[:, 1], n)
            verdict = (x > mean + nsigma * std) | (x < mean - nsigma * std)
            allp = {"key_id": pk[kept], "flow_end_s": pt[kept], "throughput": x[kept], "algo_calc": mean[kept], "stddev": std[kept],
                    "anomaly": verdict[kept].astype(np.uint8)}
            z = verdict[kept]
            for f in ROW_FIELDS:
                assert np.array_equal(bits(allp[f][z]), bits(job[f])), f
            assert job["n_points"] == pk.size and job["n_keys"] == n.size and job["keys_no_result"] == int(((n < ms) | (n < 2)).sum())
            self._want[nsigma, ms] = (job, allp)
        return self._want[nsigma, ms]


def rows_table(series, K, seed, **stage0):
    """series: (key id, day numbers, values) per key, one row per point -> a DropTable with its rows shuffled"""
    rng = np.random.default_rng(seed)
    key = np.concatenate([np.full(len(v), k, np.uint64) for k, _, v in series])
    t = np.concatenate([T_BASE + DAY * np.asarray(d, dtype=np.int64) for _, d, _ in series])
    v = np.concatenate([np.asarray(v, dtype=np.uint64) for _, _, v in series])
    o = rng.permutation(key.size)
    lengths = np.zeros(K, dtype=np.int64)
    for k, _, val in series:
        lengths[k] = len(val)
    return DropTable(key[o], t[o], v[o], K, lengths=lengths, **stage0)


# ---- part 1: every series length ----
def length_table(lengths, per_length, seed):
    """per_length keys of every length, alternately contiguous from the first day / scattered (the scattered ones alternately from day
    2 and from day 0), every second key with a dip; key ids in a shuffled order, so that a key's length does not follow from its lane"""
    rng = np.random.default_rng(seed)
    K = len(lengths) * per_length
    ids = rng.permutation(K)
    series = []
    for i, n in enumerate(lengths):
        for s in range(per_length):
            scattered = s % 2 == 1
            dip = (s // 2 + (i if per_length < 4 else 0)) % 2 == 1
            series.append((int(ids[i * per_length + s]), days_of(rng, n, scattered, 2 * ((i + s // 2) % 2)), draw_key(rng, n, dip)))
    return rows_table(series, K, seed + 1)


def short_table():
    """4 keys of every length 1 .. 300 (contiguous / scattered x plain / dip): 1200 keys over about 500 days"""
    return length_table(SHORT_LENGTHS, 4, 101)


def long_table():
    """2 keys (one contiguous, one scattered; the dip alternates) of every length 511 .. 529, 1023 .. 1041, 2049 and 4100: 80 keys"""
    return length_table(LONG_LENGTHS, 2, 202)


def assert_order_sensitive(tab, lengths):
    """the condition of this file's docstring, from the oracle alone"""
    pk, pt, x, ptr, _ = tab.points()
    n = np.diff(ptr)
    assert sorted(set(n.tolist())) == sorted(lengths)
    good = {}
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b - a >= 4 and order_sensitive(x[a:b]):
            good[b - a] = good.get(b - a, 0) + 1
    short = [m for m in lengths if m >= 4 and good.get(m, 0) < 2]
    assert not short, short


def assert_days_layout(tab):
    """half the keys contiguous from the table's first day; the others with missing days between present ones, some without the first day"""
    pk, pt, x, ptr, _ = tab.points()
    first, last, n = pt[ptr[:-1]], pt[ptr[1:] - 1], np.diff(ptr)
    holes = (last - first) // DAY + 1 - n
    contiguous = (holes == 0) & (first == T_BASE)
    assert contiguous.sum() >= n.size // 2 and ((holes >= 2) & (n >= 3)).sum() >= (n >= 3).sum() // 2 - 2
    assert ((first > T_BASE) & (holes >= 2)).sum() >= n.size // 8 and ((first == T_BASE) & (holes >= 2)).sum() >= n.size // 8
    assert (last < pt.max()).sum() >= n.size - 2            # the last day of the span is absent for all but the longest keys


# ---- part 2: key counts ----
K_EDGES = (1, 63, 64, 65, 255, 256, 257, 513)


def key_count_table(K):
    """k_drop_detect: one lane per key, wavefronts of 64, blocks of 256.  When K >= 192 the keys of the second wavefront (64 .. 127) have
    no rows at all; in every other wavefront lane 0 holds a key of 1 point and lane 63 one of 2 points (no result at the default
    min_samples); every fifth key of the rest has no rows, the others are series of 3 .. 40 points, half of them scattered.  K = 1: one
    real series."""
    rng = np.random.default_rng(1000 + K)
    series = []
    for k in range(K):
        n = 3 + (k * 7) % 38
        if K == 1:
            n = 12
        elif K >= 192 and 64 <= k < 128:
            n = 0
        elif k % 64 == 0:
            n = 1
        elif k % 64 == 63:
            n = 2
        elif k % 5 == 3:
            n = 0
        if n:
            series.append((k, days_of(rng, n, k % 2 == 1, k % 3), draw_key(rng, n, k % 4 < 2)))
    return rows_table(series, K, 2000 + K)


# ---- part 4: the sparse tables with order-sensitive values ----
def revalued(key, t, K, seed, wide=True, **stage0):
    """The rows (key, t) of a table with new values, every second key with one dipped point.
    wide: every (key, t) point's rows add up (no wrap) to a value drawn as in part 1 — uniform in [2^52, 2^53), the dip in [2^40, 2^41).
    not wide: the points uniform in [2^34, 2^35), the dip in [2^20, 2^21), every row below 2^35.  The partition form of the sparse
    Stage 0 packs value and cell into 8-byte records and hands a table with a wider value to the LSD sort (tad_stage0_retry.h:
    sparse_lsd), so stage0_path 8 and 9 are only reached with narrow values.  Their value sums are exact in any order; the order shows
    in the squared deviations (the mean is no integer), and a key is redrawn until it does — with wide values until it shows in both."""
    rng = np.random.default_rng(seed)
    o = np.lexsort((t, key))
    k, tt = key[o], t[o]
    new = np.ones(k.size, dtype=bool)
    new[1:] = (k[1:] != k[:-1]) | (tt[1:] != tt[:-1])
    point = np.cumsum(new) - 1                                   # the point of every sorted row
    P = int(point[-1]) + 1
    keys, ptr = orc.series_offsets(k[new])
    hi, lo = (52, 40) if wide else (34, 20)
    pv = np.zeros(P, dtype=np.uint64)
    for a, b, kk in zip(ptr[:-1], ptr[1:], keys):                # a key's points: redrawn until the order shows (n < 4: the first draw)
        for _ in range(200):
            pv[a:b] = rng.integers(1 << hi, 1 << (hi + 1), size=b - a, dtype=np.uint64)
            if int(kk) % 2 == 1:
                pv[rng.integers(a, b)] = rng.integers(1 << lo, 1 << (lo + 1), dtype=np.uint64)
            if b - a < 4 or order_sensitive(orc.u64_to_f64(pv[a:b]), values_too=wide):
                break
    rows_of_point = np.bincount(point, minlength=P).astype(np.uint64)
    assert rows_of_point.max() <= 8
    # the further rows of a point: wide — less than 2^39 together; narrow — an equal share each, so that every row stays below 2^35
    v = rng.integers(1 << 30, 1 << 36, size=k.size, dtype=np.uint64) if wide else (pv // rows_of_point)[point]
    rest = np.zeros(P, dtype=np.uint64)
    np.add.at(rest, point[~new], v[~new])
    v[new] = pv - rest
    assert int(v.max()) < (1 << 53 if wide else 1 << 35)
    out = np.empty_like(v)
    out[o] = v
    return DropTable(key, t, out, K, **stage0)


def share_order_sensitive(tab, values_too=True):
    """the share of the table's keys with >= 8 points whose squared-deviation sum (values_too: and value sum) differs from the left-to-right sum"""
    pk, pt, x, ptr, stats = tab.points()
    hit = [order_sensitive(x[a:b], values_too) for a, b in zip(ptr[:-1], ptr[1:]) if b - a >= 8]
    return sum(hit) / len(hit)
