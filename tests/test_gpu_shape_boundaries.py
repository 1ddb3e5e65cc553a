"""GPU: the batch job at every series length T and key count K where it picks another kernel, against the CPU oracle bit for bit.

The detect and emit kernels are chosen by the grid's shape (DESIGN.md §4 has the table):
  * T <= 64 / 128 / 192 / 256: k_dbscan_list_wave<PPL> and k_emit_dbscan_wave<PPL>, PPL = 1 .. 4; lane l holds buckets l + 64 j
  * T <= 256 wave list, then k_dbscan_sorted in LDS up to 4096 points, then per-workgroup rows of global scratch; the LDS form
    strides its grid beyond 2048 listed keys, the row form beyond sort_blocks(g) = 1024, the wave list beyond 32768
  * k_dbscan_list_wave walks the smaller of {core, non-core} points of a key to find the reachable ones
  * a wavefront per key iff T >= 512 and K <= 8192 (coop_shape: sigma / count walk, flag count, emit, DBSCAN scan)
  * k_key_sigma reads its reciprocal table from LDS iff T <= 4095

Every case sits on one of these edges, and what puts it there — the noise position in every lane of every slot, border points in
both reach branches, the number of listed keys, n_buckets == T — is asserted from the oracle before the engine is asked.  The
DBSCAN cases A to C run under the direct scatter and under the partition path with the write-combining pass (settle mode exists
only there: a listed key's series is then read from the grid, from the copy behind the work list or from the copy behind the
redo list); EWMA's detect and emit do not depend on Stage 0 and run under the default plan.

The tables are small and built here from seeded numpy and orc.mix64; the builders are plain functions, usable without a GPU."""
import functools

import numpy as np
import pytest

from oracle import tad_oracle as orc
from job_helpers import check_job

pytestmark = pytest.mark.gpu

EPS = 250_000_000            # the detector's defaults (anomaly_detection.py:325-349)
MIN_SAMPLES = 4
T_BASE, T_STEP = orc.SYNTH_T_BASE, orc.SYNTH_T_STEP
U64 = np.uint64
DENSE_PATHS = (1, 2, 3)      # stage0_path: direct scatter, partition + sort pass, partition + write-combining pass

WAVE_T = (63, 64, 65, 127, 128, 129, 160, 191, 192, 193, 255, 256)


@pytest.fixture(params=["v1", "v2wc"])
def stage0(request, engine):
    """v1 = direct atomic scatter: every listed key is gathered from the grid.  v2wc = partition + LDS tiles with the
    write-combining pass, forced on these small tables: DBSCAN jobs run the tile pass in settle mode."""
    engine.set_plan(stage0=request.param[:2], partition_pass="wc" if request.param == "v2wc" else "sort")
    yield request.param
    engine.set_plan()


@pytest.fixture(scope="module", autouse=True)
def oracle_once():
    """check_job asks the oracle for the job it compares with, and both Stage-0 strategies ask for the same jobs: the oracle runs
    once per (table, detector, parameters).  The builders below are cached, so the identity of the key and value columns names
    the table.  The results are read, never written."""
    real, memo = orc.run_job, {}

    def run_job(algo, key_id, flow_end_s, value, **kw):
        try:
            tag = (algo, id(key_id), id(value)) + tuple(sorted(kw.items()))
            hash(tag)
        except (TypeError, ValueError):     # a column among the arguments: not one of this module's shared jobs
            return real(algo, key_id, flow_end_s, value, **kw)
        if tag not in memo:
            memo[tag] = (real(algo, key_id, flow_end_s, value, **kw), key_id, value)      # (the columns stay alive: ids are not reused)
        return memo[tag][0]
    orc.run_job = run_job
    yield
    orc.run_job = real


def _rows(key, bucket, value, seed):
    """the three columns of a table, rows in a seeded arbitrary order"""
    key, bucket, value = (np.concatenate(x) for x in (key, bucket, value))
    o = np.random.default_rng(seed).permutation(key.size)
    return (np.ascontiguousarray(key[o].astype(U64)), np.ascontiguousarray(T_BASE + T_STEP * bucket[o].astype(np.int64)),
            np.ascontiguousarray(value[o].astype(U64)))


def _h(k, t, salt):
    return orc.mix64(np.asarray(k, dtype=U64) * U64(1_000_003) + np.asarray(t, dtype=U64) * U64(8191) + U64(salt))


def series_stats(key, t, v, op="max"):
    """(keys, ptr, values as double, max - min, point count) of every key's series, from the oracle's Stage 0"""
    pk, pt, pv = orc.stage0(key, t, v, op)
    keys, ptr = orc.series_offsets(pk)
    x = orc.u64_to_f64(pv)
    return keys, ptr, x, np.maximum.reduceat(x, ptr[:-1]) - np.minimum.reduceat(x, ptr[:-1]), np.diff(ptr)


def listed_keys(key, t, v, op="max", eps=EPS, min_samples=MIN_SAMPLES):
    """how many keys the scan lists for the exact predicate: spread beyond eps or fewer than min_samples points (as
    tests/test_gpu_parameters.py: spread_P)"""
    _, _, _, spread, n = series_stats(key, t, v, op)
    return int(((spread > eps) | (n < min_samples)).sum())


# ------------------------------------------------------------------ A: every bucket position of the wave-list kernels
@functools.lru_cache(maxsize=None)
def spike_table(T, second_rows=False, overflow=False):
    """K = T + 7 keys on T buckets.  Key k < T: a dense cluster (base 1e9 + (k % 13) * 1e6, jitter below 9e5, a fifth of the cells
    absent) and one spike base + 10 eps at bucket k % T, the key's only noise point: over the keys the noise point visits every
    lane of every 64-bucket slot, bucket T - 1 and the partial last slot included.  A key with one noise point cannot see the
    emit's running row offset, so one of the seven other keys has an isolated point in the first and the last lane of every
    slot (edge_buckets): rows in every slot, each behind those of the slots before.  The other six have no spike: plain
    clusters, one on every bucket, one key without rows, one with three points, one with a single point at bucket T - 1.
    second_rows: a tenth of the cluster cells get a second row of 1 .. 1000, so a cell's sum is not its max.
    overflow: about 3 in 1000 values lie in [2^50, 2^63) (the overflow list of the packed records)."""
    K = T + 7
    kk, tt = np.meshgrid(np.arange(K, dtype=np.int64), np.arange(T, dtype=np.int64), indexing="ij")
    kk, tt = kk.ravel(), tt.ravel()
    base = 1_000_000_000 + (kk % 13) * 1_000_000
    val = base + (_h(kk, tt, 1) % U64(900_000)).astype(np.int64)
    present = _h(kk, tt, 2) % U64(5) != 0
    spike = (kk < T) & (tt == kk % T)
    val = np.where(spike, base + 10 * EPS, val)
    present |= spike
    present[kk == T + 1] = False                                         # no rows at all
    present[kk == T + 2] = np.isin(tt[kk == T + 2], (1, T // 2, T - 2))  # three points: all noise
    present[kk == T + 3] = True                                          # every bucket
    present[kk == T + 4] = tt[kk == T + 4] == T - 1                      # a single point, in the last bucket
    edge = (kk == T + 5) & np.isin(tt, edge_buckets(T))                  # noise at both ends of every slot
    val = np.where(edge, base + (20 + 3 * tt) * EPS, val)
    present |= edge
    key, bucket, value = [kk[present]], [tt[present]], [val[present]]
    if second_rows:
        twice = present & ~spike & (_h(kk, tt, 3) % U64(10) == 0)
        key.append(kk[twice]); bucket.append(tt[twice]); value.append(1 + (_h(kk, tt, 4)[twice] % U64(1000)).astype(np.int64))
    k, t, v = _rows(key, bucket, value, seed=T)
    if overflow:
        rng = np.random.default_rng(11)
        sel = rng.random(v.size) < 0.003
        v = v.copy()
        v[sel] = rng.integers(2**50, 2**63, size=int(sel.sum()), dtype=np.uint64)
    return k, t, v, K


def edge_buckets(T):
    return sorted({b for b in (0, 63, 64, 127, 128, 191, 192, 255) if b < T} | {T - 1})


def assert_one_noise_point_per_key_in_every_bucket(want, T):
    pk, pt, _ = want["points"]
    noise = want["anomaly_all"] & (pk < T)
    nk, nb = pk[noise].astype(np.int64), (pt[noise] - T_BASE) // T_STEP
    assert nk.tolist() == list(range(T))                # exactly one per key, keys ascending
    assert (nb == nk % T).all() and sorted(nb.tolist()) == list(range(T))
    assert set((nb // 64).tolist()) == set(range((T + 63) // 64)) and nb.max() == T - 1
    # the other keys: the three-point key, the single point and the points at the slots' ends are noise, the clusters are not
    rest = want["anomaly_all"] & (pk >= T)
    assert sorted(set(pk[rest].tolist())) == [T + 2, T + 4, T + 5] and rest.sum() == 4 + len(edge_buckets(T))
    assert ((pt[rest & (pk == T + 5)] - T_BASE) // T_STEP).tolist() == edge_buckets(T)


@pytest.mark.parametrize("agg", ["", "svc"], ids=["max", "sum"])
@pytest.mark.parametrize("T", WAVE_T)
def test_wave_list_noise_point_in_every_lane_of_every_slot(engine, stage0, T, agg):
    """k_dbscan_list_wave<PPL> and k_emit_dbscan_wave<PPL>, PPL = 1 .. 4, at both ends of every PPL's range: a noise point in
    each bucket, so a wrong slot offset, lane mask or row offset of any slot shows as a wrong row."""
    k, t, v, K = spike_table(T, second_rows=bool(agg))
    want = orc.run_job("DBSCAN", k, t, v, agg_flow=agg)
    assert_one_noise_point_per_key_in_every_bucket(want, T)
    assert listed_keys(k, t, v, "sum" if agg else "max") == T + 3        # every spike key, the three-point key, the single point, the slots' ends
    if agg:
        assert (want["points"][2] != orc.stage0(k, t, v, "max")[2]).sum() > T      # sums that are not the max
    res, _ = check_job(engine, "DBSCAN", k, t, v, K, agg_flow=agg)
    assert res.stats["n_buckets"] == T and res.stats["n_keys"] == K - 1
    assert res.stats["stage0_path"] == (1 if stage0 == "v1" else 3)


def test_wave_list_three_slots_with_values_on_the_overflow_list(engine, stage0):
    """T = 160 (PPL = 3) with values beyond the packed records' range: in settle mode their keys go to the redo list, the list
    kernels read such a key's series behind the redo list and its flagged cells from the grid."""
    T = 160
    k, t, v, K = spike_table(T, overflow=True)
    want = orc.run_job("DBSCAN", k, t, v, agg_flow="")
    pk, _, pv = want["points"]
    big = pv >= U64(2**50)
    assert 20 < big.sum() < 200 and want["anomaly_all"][big].all()
    assert np.unique(pk[big]).size > 20 and set(((want["points"][1][big] - T_BASE) // T_STEP // 64).tolist()) == {0, 1, 2}
    assert T < want["n_anomalies"] < want["n_points"] // 20
    res, _ = check_job(engine, "DBSCAN", k, t, v, K, agg_flow="")
    assert res.stats["n_buckets"] == T
    assert res.stats["stage0_path"] == (1 if stage0 == "v1" else 3)


# ------------------------------------------------------------------ B: both reach branches, with border points
@functools.lru_cache(maxsize=None)
def reach_table(T):
    """200 keys of two kinds, alternating, centre c = 1e9 + 1e6 (k % 17).
    Dense keys: a cluster of at least 150 points in [c, c + 0.4 eps], one more cluster point at c + 0.6 eps, a border point at
    c + 1.5 eps (its neighbours: itself and the point at c + 0.6 eps — not core, within eps of a core point) and two isolated
    points: far more core points than others.
    Sparse keys: c, c, c, c + 0.9 eps (all core), a border point at c + 1.8 eps and 20 to 27 mutually isolated points: more
    points that are not core than core points.
    The buckets of a key's special points are drawn per key, so over a kind they visit every 64-bucket slot."""
    K = 200
    key, bucket, value = [], [], []
    for k in range(K):
        c = 1_000_000_000 + 1_000_000 * (k % 17)
        order = np.argsort(_h(np.full(T, k), np.arange(T), 5), kind="stable")       # this key's buckets in an order of its own
        if k % 2 == 0:
            n = T if k == 0 else 154 + int(_h(k, 0, 6) % U64(T - 154 - 8))        # key 0 fills every bucket: the lattice's ends
            b = order[:n]
            x = c + (_h(np.full(n, k), b, 7) % U64(4 * EPS // 10 + 1)).astype(np.int64)
            x[0], x[1], x[2], x[3] = c + 6 * EPS // 10, c + 15 * EPS // 10, c + 5 * EPS, c + 8 * EPS
        else:
            iso = 20 + k % 8
            b = order[:5 + iso]
            x = np.concatenate([[c, c, c, c + 9 * EPS // 10, c + 18 * EPS // 10], c + 5 * EPS + 3 * EPS * np.arange(iso)]).astype(np.int64)
        key.append(np.full(b.size, k)); bucket.append(b); value.append(x)
    return _rows(key, bucket, value, seed=1000 + T) + (K,)


def point_kinds(x, eps, min_samples):
    """(core, border, noise) of one key's values by the oracle's definition (oracle.tad_oracle.dbscan_noise_1d)"""
    d = np.abs(x[:, None] - x[None, :]) <= eps
    core = d.sum(axis=1) >= min_samples
    reach = (d & core[None, :]).any(axis=1)
    return core, ~core & reach, ~core & ~reach


@pytest.mark.parametrize("eps,min_samples", [(0, 0), (5e5, 2)], ids=["defaults", "eps5e5-ms2"])
@pytest.mark.parametrize("T", [192, 256])
def test_wave_list_both_reach_branches_with_border_points(engine, stage0, T, eps, min_samples):
    """k_dbscan_list_wave walks the non-core points of a key when they are fewer than its core points and the core points
    otherwise.  Both branches must run at PPL = 3 and 4, each with a border point (what only the reach test keeps from being
    noise) and a noise point in every slot."""
    k, t, v, K = reach_table(T)
    pk, pt, pv = orc.stage0(k, t, v, "max")
    keys, ptr = orc.series_offsets(pk)
    x, b = orc.u64_to_f64(pv), (pt - T_BASE) // T_STEP
    slots = {"few_rest": [set(), set()], "few_core": [set(), set()]}       # per branch: slots with a border point, with a noise point
    n_keys = {"few_rest": 0, "few_core": 0}
    noise_all = np.zeros(pk.size, dtype=bool)
    for a, e in zip(ptr[:-1], ptr[1:]):
        core, border, noise = point_kinds(x[a:e], float(EPS), MIN_SAMPLES)
        noise_all[a:e] = noise
        branch = "few_rest" if (e - a) - core.sum() < core.sum() else "few_core"      # n_rest < n_core, as the kernel decides
        n_keys[branch] += 1
        slots[branch][0] |= set((b[a:e][border] // 64).tolist())
        slots[branch][1] |= set((b[a:e][noise] // 64).tolist())
        assert border.sum() == 1 and noise.sum() >= 2
    want = orc.run_job("DBSCAN", k, t, v, agg_flow="")
    assert (noise_all == want["anomaly_all"]).all()
    assert n_keys == {"few_rest": K // 2, "few_core": K // 2}
    every_slot = set(range(T // 64))
    assert all(s == every_slot for pair in slots.values() for s in pair), slots
    assert listed_keys(k, t, v) == K
    if eps:          # away from the defaults the clusters break up: noise and clustered points in quantity, on every key
        want = orc.run_job("DBSCAN", k, t, v, agg_flow="", eps=eps, min_samples=min_samples)
        assert want["n_points"] // 4 < want["n_anomalies"] < 3 * want["n_points"] // 4
    res, _ = check_job(engine, "DBSCAN", k, t, v, K, agg_flow="", eps=eps, min_samples=min_samples)
    assert res.stats["n_buckets"] == T
    assert res.stats["stage0_path"] == (1 if stage0 == "v1" else 3)


# ------------------------------------------------------------------ C: the sorted-window kernel as a job with many listed keys
def _short_series(rng, keys, T, lo, hi, clustered):
    """A share `clustered` of the keys gets five or six points: four within eps / 2 of each other (core points) and, BELOW them,
    one or two isolated ones — the key's smallest value is noise.  The other keys get lo .. hi points spread over 12 eps."""
    key, bucket, value = [], [], []
    for k in keys:
        if rng.random() < clustered:
            n = int(rng.integers(5, 7))
            x = np.concatenate([2_000_000_000 + 3 * EPS * np.arange(n - 4), 2_000_000_000 + 20 * EPS + rng.integers(0, EPS // 2, size=4)])
            x = x[rng.permutation(n)]
        else:
            n = int(rng.integers(lo, hi + 1))
            x = 2_000_000_000 + rng.integers(0, 12 * EPS, size=n)
        key.append(np.full(n, k))
        bucket.append(rng.choice(T, size=n, replace=False))
        value.append(x)
    return key, bucket, value


def _long_series(rng, k, T, n, scale):
    """n points of key k: 4e9 * scale +- 2.7e9 * scale, every 97th point a spike of four times its value.  scale 1 on some
    hundred points is one cluster and its spikes; larger scales thin it out into core, border and noise points."""
    b = np.sort(rng.choice(T, size=n, replace=False)) if n < T else np.arange(T)
    x = scale * (4_000_000_000 + rng.integers(-2_700_000_000, 2_700_000_000, size=n))
    x[::97] *= 4
    return np.full(n, k), b, x


@functools.lru_cache(maxsize=None)
def sorted_lds_table():
    """K = 2200, T = 257: 41 keys with series of 200 to 257 points at four spreads — ten of them among the first keys, so that
    their workgroups of k_dbscan_sorted go on to a short entry 2048 places down the list — and 1 to 6 points on every other key,
    most of them a cluster of four above one or two isolated points"""
    K, T = 2200, 257
    rng = np.random.default_rng(257)
    long_keys = [k for k in range(K) if k % 73 == 0 or 1 <= k <= 10]
    key, bucket, value = _short_series(rng, [k for k in range(K) if k not in set(long_keys)], T, 1, 6, 0.97)
    for i, k in enumerate(long_keys):
        kk, b, x = _long_series(rng, k, T, T if i % 3 == 0 else int(rng.integers(200, T)), (1, 3, 10, 30)[i % 4])
        key.append(kk); bucket.append(b); value.append(x)
    return _rows(key, bucket, value, seed=2200) + (K, T, len(long_keys))


@functools.lru_cache(maxsize=None)
def sorted_rows_table():
    """K = 1100, T = 4097 (past the 4096 points of the LDS form: rows of global scratch, 8192 points each): 12 keys with 3500
    to 4097 points at three spreads, 1 to 6 points on every other key, most of them a cluster of four above one or two isolated
    points"""
    K, T = 1100, 4097
    rng = np.random.default_rng(4097)
    long_keys = [0, 1, 2, 3, 5, 8, 100, 500, 1023, 1024, 1098, 1099]
    key, bucket, value = _short_series(rng, [k for k in range(K) if k not in set(long_keys)], T, 1, 6, 0.97)
    for i, k in enumerate(long_keys):
        kk, b, x = _long_series(rng, k, T, T if i % 4 == 0 else int(rng.integers(3500, T)), (1, 30, 100)[i % 3])
        key.append(kk); bucket.append(b); value.append(x)
    return _rows(key, bucket, value, seed=1100) + (K, T, len(long_keys))


@functools.lru_cache(maxsize=None)
def thin_table(K):
    """T = 512 and 8193 keys, of which K are kept: 1 to 3 points on most keys, a cluster of four above one or two isolated points
    on a tenth of them, 300 to 512 points on every 199th and on the last one (key 8192).  With K = 8193 a lane walks a key, with K = 8192 a wavefront: the same rows without key 8192."""
    T = 512
    rng = np.random.default_rng(8193)
    long_keys = [k for k in range(8193) if k % 199 == 0 or k == 8192]
    key, bucket, value = _short_series(rng, [k for k in range(8193) if k not in set(long_keys)], T, 1, 3, 0.1)
    for i, k in enumerate(long_keys):
        kk, b, x = _long_series(rng, k, T, T if i % 5 == 0 else int(rng.integers(300, T)), (1, 3, 10, 30)[i % 4])
        key.append(kk); bucket.append(b); value.append(x)
    k, t, v = _rows(key, bucket, value, seed=8193)
    keep = k < U64(K)
    return np.ascontiguousarray(k[keep]), np.ascontiguousarray(t[keep]), np.ascontiguousarray(v[keep]), K, T, sum(1 for q in long_keys if q < K)


@functools.lru_cache(maxsize=None)
def all_noise_table():
    """K = 40000, T = 70: 1 to 3 points on every key.  Every key is listed and every point is noise."""
    K, T = 40000, 70
    rng = np.random.default_rng(70)
    n = rng.integers(1, 4, size=K)
    key = np.repeat(np.arange(K), n)
    bucket = (np.repeat(rng.integers(0, T, size=K), n) + np.concatenate([np.arange(m) for m in n]) * 23) % T      # distinct buckets per key
    value = 1_000_000_000 + rng.integers(0, 12 * EPS, size=key.size)
    return _rows([key], [bucket], [value], seed=40000) + (K, T)


def check_many_listed(engine, stage0, table, min_listed, long_keys, workgroups=0):
    """workgroups: of a kernel that gives entry e, e + workgroups, ... of the work list to one workgroup.  The order of the list
    is up to the scheduler, so the table must make a workgroup carry state from one key to the next IN ANY ORDER: more entries
    have a successor on their workgroup than there are keys without core points (nothing to carry: no core prefix) and keys whose
    smallest value is not noise (the first sorted point is where a stale prefix shows) taken together."""
    k, t, v, K, T = table[:5]
    keys, ptr, x, spread, n = series_stats(k, t, v)
    listed = (spread > EPS) | (n < MIN_SAMPLES)
    assert min_listed < listed.sum() <= K
    assert ((n >= 200) & listed).sum() == (n >= 200).sum() == long_keys      # the long series are all listed ...
    assert (listed & (n <= 6)).sum() > min_listed - long_keys                # ... among that many short ones
    want = orc.run_job("DBSCAN", k, t, v, agg_flow="")
    noise = want["anomaly_all"]
    noisy = np.add.reduceat(noise, ptr[:-1])
    if workgroups:
        no_core = listed & (noisy == n)
        min_clustered = listed & (np.add.reduceat(noise & (x == np.repeat(np.minimum.reduceat(x, ptr[:-1]), n)), ptr[:-1]) == 0)
        assert listed.sum() - workgroups > no_core.sum() + min_clustered.sum() + 20
    with engine.plan(sparse="never"):
        res, want = check_job(engine, "DBSCAN", k, t, v, K, agg_flow="")
    assert res.stats["n_buckets"] == T and res.stats["n_keys"] == K
    assert res.stats["stage0_path"] in ((1,) if stage0 == "v1" else (2, 3))
    return want, n, noisy


def test_sorted_windows_in_lds_stride_over_long_and_short_entries(engine, stage0):
    """k_dbscan_sorted's LDS form launches 2048 workgroups: with more listed keys a workgroup handles several entries one after
    the other, here a series of hundreds of points and then one of a few — whatever the first left in xs / bk / lo / hi / cp,
    in the point count and in the prefix carry must not reach the second."""
    table = sorted_lds_table()
    want, n, noisy = check_many_listed(engine, stage0, table, 2048, table[5], workgroups=2048)
    assert ((n >= 200) & (noisy > 0) & (noisy < n)).sum() == table[5] == 41      # every long series has noise and clustered points
    assert (n < MIN_SAMPLES).sum() > 20


def test_sorted_windows_in_global_rows_stride_over_long_and_short_entries(engine, stage0):
    """series of more than 4096 buckets: k_dbscan_sorted works in per-workgroup rows of global scratch, sort_blocks(g) = 1024
    of them here, so with more listed keys a row is used again after a long key"""
    table = sorted_rows_table()
    want, n, noisy = check_many_listed(engine, stage0, table, 1024, table[5], workgroups=1024)
    assert n.max() == 4097 and ((n >= 3500) & (noisy > 0) & (noisy < n)).sum() == table[5] == 12
    assert (n < MIN_SAMPLES).sum() > 10


@pytest.mark.parametrize("K", [8193, 8192], ids=["lane_per_key", "wavefront_per_key"])
def test_dbscan_scan_on_either_side_of_8192_keys(engine, stage0, K):
    """T = 512: k_dbscan_scan<false, false> (a lane per key, K = 8193) and its wavefront-per-key form (K = 8192) on the same
    rows, both listing more than 2048 keys for k_dbscan_sorted"""
    table = thin_table(K)
    want, n, noisy = check_many_listed(engine, stage0, table, 2048, table[5])
    assert (n <= 3).sum() > 7000 and ((n <= 6) & (noisy < n)).sum() > 500       # some hundred short keys with core points
    if K == 8193:
        assert want["points"][0][-1] == 8192 and thin_table(8192)[0].size == table[0].size - np.diff(want["ptr"])[-1]


def test_wave_list_strides_over_40000_listed_keys(engine, stage0):
    """more list entries than the 32768 wavefronts of k_dbscan_list_wave's grid, most of them past compact_cap(g) = 5000, on the
    dense path: every point of the table is noise"""
    table = all_noise_table()
    want, _, _ = check_many_listed(engine, stage0, table, 32768, 0)
    assert listed_keys(*table[:3]) == 40000 and want["n_anomalies"] == want["n_points"] > 70000


# ------------------------------------------------------------------ D: EWMA and sigma at the coop and reciprocal-table edges
@functools.lru_cache(maxsize=None)
def holey_table(K, T, n_rows):
    """orc.synth_rows with a fifth of the (key, time) cells absent; key 0 keeps the first and the last bucket"""
    k, t, v = orc.synth_rows(17, n_rows, K, T)
    keep = (orc.mix64(k * U64(977) + t.astype(U64)) % U64(5)) != 0
    k, t, v = k[keep], t[keep], v[keep]
    ends = np.array([0, T - 1], dtype=np.int64)
    return (np.ascontiguousarray(np.concatenate([k, np.zeros(2, dtype=U64)])), np.ascontiguousarray(np.concatenate([t, T_BASE + T_STEP * ends])),
            np.ascontiguousarray(np.concatenate([v, np.array([1_500_000_000, 1_600_000_000], dtype=U64)])))


EWMA_SHAPES = [(5, 511, 0), (5, 512, 0), (5, 513, 0), (5, 576, 0), (5, 4095, 0), (5, 4096, 0), (5, 4097, 0),
               (8192, 512, 1_500_000), (8193, 512, 1_500_000), (8193, 4096, 375_000)]


@pytest.mark.parametrize("K,T,n_rows", EWMA_SHAPES, ids=["%dx%d" % s[:2] for s in EWMA_SHAPES])
def test_ewma_job_at_the_coop_and_reciprocal_table_edges(engine, K, T, n_rows):
    """k_key_sigma, the count walk and the emit with a lane and with a wavefront per key (T 511 / 512 / 513, K 8192 / 8193; T = 576:
    whole 64-bucket blocks only in the coop walk), the reciprocal table in LDS and not (T 4095 / 4096 / 4097); 8193 x 4096 is the
    lane-per-key form without the table in LDS.  At the default alpha and at 0.3."""
    k, t, v = holey_table(K, T, n_rows or 4 * K * T)
    with engine.plan(sparse="never"):          # (8193 x 4096 holds 3e5 rows: thin enough for the sparse path)
        for alpha in (0, 0.3):
            res, want = check_job(engine, "EWMA", k, t, v, K, agg_flow="svc", alpha=alpha)
            assert res.stats["n_buckets"] == T and res.stats["n_keys"] == K
            assert res.stats["stage0_path"] in DENSE_PATHS
            assert want["n_anomalies"] > 100 and want["has_sigma"].all()
    n = np.diff(want["ptr"])
    if n_rows == 0:
        assert n.min() > T // 2 and (n < T).all()          # long series with holes
    else:
        assert n.min() >= 2 and n.max() > 50


@pytest.mark.parametrize("T", [511, 512, 513])
def test_dbscan_job_on_either_side_of_the_coop_edge(engine, T):
    """the DBSCAN scan, the flag count and the emit with a lane per key (T = 511) and a wavefront per key (512, 513)"""
    k, t, v = holey_table(5, T, 4 * 5 * T)
    res, want = check_job(engine, "DBSCAN", k, t, v, 5, agg_flow="svc")
    assert res.stats["n_buckets"] == T and 0 < want["n_anomalies"] < want["n_points"] // 10


# ------------------------------------------------------------------ E: the series entry point
def test_series_dbscan_at_every_length_class_edge(engine):
    """series_dbscan_anomaly at both ends of every PPL's range, at the first length of k_dbscan_sorted and on either side of its
    4096 LDS points; three times the spread of test_series_long_dbscan_sorted_windows, so that short series have noise too"""
    rng = np.random.default_rng(5)
    for n in (64, 65, 128, 129, 192, 193, 256, 257, 4096, 4097):
        x = (4_000_000_000 + rng.integers(-2_700_000_000, 2_700_000_000, size=n)).astype(np.uint64)
        x[::29] *= np.uint64(4)
        want = orc.dbscan_noise_1d(orc.u64_to_f64(x))
        assert 2 <= want.sum() < n // 2, n
        assert (engine.series_dbscan_anomaly(x) == want).all(), n
