"""GPU: the drop detector (TAD_ALGO_DROP / tad_series_drop) against the reference UDF's golden, its outputs on seeded
series (tests/golden/drop_outputs.json) and the oracle on synthetic tables.  Bit-exact: the kernel sums in numpy's
pairwise order."""
import json
import os

import numpy as np
import pytest

from oracle import drop_oracle as dro
from oracle import tad_oracle as orc
from theia_amd import anomaly_detection as ad
from theia_amd import drop_detection as dd

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drop_outputs.json")


@pytest.fixture(scope="module")
def drop_golden():
    with open(GOLD) as f:
        return json.load(f)


def test_end_partition_like_the_reference_unit_test(engine, drop_golden):
    # drop_detection_udf_test.py:141-171, same calls, same exact-equality assertions
    ad.set_engine(engine)
    try:
        det = dd.DropDetection()
        for i, x in enumerate(drop_golden["series"]["reference_test"]["x"]):
            next(det.process(job_type="initial", detection_id=drop_golden["detection_id"], endpoint="antrea-test/Pod-A",
                             direction="ingress", date="2022-01-%02d" % (i + 1), drop_number=x))
        results = list(det.end_partition())
        assert len(results) == len(drop_golden["expected_result"]) == 1
        _, detection_id, _, endpoint, direction, avg_drop, stdev_drop, date, number = results[0]
        assert detection_id == drop_golden["detection_id"]
        assert [endpoint, direction, avg_drop, stdev_drop, date, number] == drop_golden["expected_result"][0]
    finally:
        ad.set_engine(None)


def test_series_equal_reference_udf_outputs_bit_for_bit(engine, drop_golden):
    for name, e in drop_golden["series"].items():
        out = engine.series_drop(e["x"])
        if len(e["x"]) < 3:
            assert out is None and e["rows"] == [], name
            continue
        mean, std, verdict = out
        assert np.flatnonzero(verdict).tolist() == [int(r[2].split("-")[1]) for r in e["rows"]], name
        for r in e["rows"]:
            assert r[0] == mean and r[1] == std, (name, r[:2], mean, std)
        omean, ostd, overdict = dro.drop_detection_series(e["x"])
        assert (mean, std) == (omean, ostd) and (verdict == overdict).all(), name


def check_job(engine, key, day, drops, K, nsigma=0.0, min_samples=0):
    """the job's rows and, with emit_all, every point of every key with enough samples, against the oracle; 0 = the detector's default"""
    okw = {k: val for k, val in (("n_sigma", nsigma), ("min_samples", min_samples)) if val}
    kw = dict(drop_nsigma=nsigma, drop_min_samples=min_samples)
    want = dro.run_job(key, day, drops, **okw)
    res = engine.run("DROP", key, day, drops, K, agg_flow="svc", **kw)
    assert res.stats["keys_no_result"] == want["keys_no_result"] and res.stats["n_points"] == want["n_points"]
    assert res.n_rows == want["n_anomalies"] > 0
    for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
        assert (res[f] == want[f]).all(), f
    # emit_all: every point of every key with >= min_samples samples, verdict column consistent
    allp = engine.run("DROP", key, day, drops, K, agg_flow="svc", emit_all=True, **kw)
    assert int(allp["anomaly"].sum()) == want["n_anomalies"]
    upper = allp["algo_calc"] + (nsigma or 3.0) * allp["stddev"]
    lower = allp["algo_calc"] - (nsigma or 3.0) * allp["stddev"]
    assert (((allp["throughput"] > upper) | (allp["throughput"] < lower)) == allp["anomaly"].astype(bool)).all()
    # ... and mean and std of EVERY emitted key are the oracle's bits, the keys without an anomalous day included
    pk, pt, pv = orc.stage0(key, day, drops, "sum")
    keys, ptr = orc.series_offsets(pk)
    x = orc.u64_to_f64(pv)
    n = np.diff(ptr)
    kept = n >= (min_samples or dro.MIN_SAMPLES)
    stats = np.array([dro.drop_stats(x[a:b]) if ok else (0.0, 0.0) for a, b, ok in zip(ptr[:-1], ptr[1:], kept)])
    rows = np.repeat(kept, n)
    assert allp.n_rows == int(rows.sum()) and int((~kept).sum()) == want["keys_no_result"]
    assert (allp["key_id"] == pk[rows]).all() and (allp["flow_end_s"] == pt[rows]).all() and (allp["throughput"] == x[rows]).all()
    assert (allp["algo_calc"] == np.repeat(stats[:, 0], n)[rows]).all()
    assert (allp["stddev"] == np.repeat(stats[:, 1], n)[rows]).all()
    return res, want


def poisson_table(n_rows, K, T):
    rng = np.random.default_rng(n_rows)
    key = rng.integers(0, K, size=n_rows).astype(np.uint64)
    day = 19000 + rng.integers(0, T, size=n_rows).astype(np.int64)          # one bucket per day
    drops = rng.poisson(3.0, size=n_rows).astype(np.uint64)
    spike = rng.random(n_rows) < 0.002
    drops = np.where(spike, drops * np.uint64(200) + np.uint64(500), drops)
    return key, day, drops


@pytest.mark.parametrize("n_rows,K,T", [(50000, 300, 40), (400000, 2000, 365), (30000, 4000, 30)])
def test_job_matches_oracle(engine, n_rows, K, T):
    check_job(engine, *poisson_table(n_rows, K, T), K)


@pytest.mark.parametrize("nsigma,min_samples", [(2.5, 0), (1.0, 5), (3.0, 10)])
def test_job_nsigma_and_min_samples_match_oracle(engine, nsigma, min_samples):
    """drop_nsigma and drop_min_samples away from their defaults (3 sigma, 3 samples) on the smallest table: its 4000 keys have 1 to
    about 15 days each, so min_samples 5 and 10 drop keys that the default keeps"""
    key, day, drops = poisson_table(30000, 4000, 30)
    res, want = check_job(engine, key, day, drops, 4000, nsigma, min_samples)
    usual = dro.run_job(key, day, drops)
    assert (want["n_anomalies"], want["keys_no_result"]) != (usual["n_anomalies"], usual["keys_no_result"])
    if min_samples:
        assert 100 < want["keys_no_result"] - usual["keys_no_result"] and want["keys_no_result"] < 3900
    if nsigma >= 2.5:
        assert np.unique(want["key_id"]).size < (want["n_keys"] - want["keys_no_result"]) // 2      # most emitted keys have no anomalous day


@pytest.mark.parametrize("nsigma", [0.0, 1.0])
def test_job_long_series_of_large_counts(engine, nsigma):
    """Series of 130, 257 and 600 days with counts in [2^40, 2^44]: numpy's pairwise sum recurses once at 130 days and twice at 257
    and 600.  Small Poisson counts add up exactly in any order and cannot tell one order from another; 600 counts just below 2^44
    add up to more than 2^53, where the order of the additions shows in the mean itself (asserted below: a left-to-right sum gives
    another value), and squared deviations of 2^80 and more show it in the standard deviation of most keys."""
    rng = np.random.default_rng(77)
    lengths = [130, 257, 600, 600, 257, 130]
    K = len(lengths)
    key = np.repeat(np.arange(K, dtype=np.uint64), lengths)
    day = 19000 + np.concatenate([np.arange(n) for n in lengths]).astype(np.int64)
    high = np.repeat(np.array(lengths) == 600, lengths)            # the long series: counts just below 2^44, rare dips
    drops = np.where(high, rng.integers(2**44 - 2**44 // 32, 2**44, size=key.size), rng.integers(2**40, 2**41, size=key.size))
    spike = rng.random(key.size) < 0.02
    drops = np.where(spike, np.where(high, rng.integers(2**40, 2**41, size=key.size), rng.integers(2**43, 2**44, size=key.size)), drops)
    drops = drops.astype(np.uint64)
    assert drops.min() >= 2**40 and drops.max() < 2**44
    order = rng.permutation(key.size)
    key, day, drops = key[order], day[order], drops[order]
    pk, pt, pv = orc.stage0(key, day, drops, "sum")
    keys, ptr = orc.series_offsets(pk)
    x = orc.u64_to_f64(pv)
    assert np.diff(ptr).tolist() == lengths
    left_to_right = [float(np.cumsum(x[a:b])[-1]) for a, b in zip(ptr[:-1], ptr[1:])]
    differs = [dro.pairwise_sum(x[a:b]) != s for a, b, s in zip(ptr[:-1], ptr[1:], left_to_right)]
    assert differs == [n == 600 for n in lengths]
    squares = [(dro.drop_stats(x[a:b])[0] - x[a:b]) ** 2 for a, b in zip(ptr[:-1], ptr[1:])]
    print("keys whose sum of squared deviations depends on the order:", [dro.pairwise_sum(sq) != float(np.cumsum(sq)[-1]) for sq in squares])
    assert sum(dro.pairwise_sum(sq) != float(np.cumsum(sq)[-1]) for sq in squares) >= K // 2
    # (one more key with a single day: no result)
    res, want = check_job(engine, np.append(key, np.uint64(K)), np.append(day, 19000), np.append(drops, np.uint64(2**40)), K + 1, nsigma)
    assert want["keys_no_result"] == 1 and np.unique(want["key_id"]).size == K


def test_table_function(engine):
    ad.set_engine(engine)
    try:
        ep = ["ns/a"] * 12 + ["ns/b"] * 12 + ["10.0.0.9"] * 2
        di = ["ingress"] * 12 + ["egress"] * 12 + ["ingress"] * 2
        date = ["2022-03-%02d" % (i + 1) for i in range(12)] * 2 + ["2022-03-01", "2022-03-02"]
        num = [3, 2, 4, 3, 2, 90, 3, 4, 2, 3, 4, 2] + [5] * 12 + [1, 100]
        rows = dd.drop_detection_table(ep, di, date, num, detection_id="d1")
        assert len(rows) == 1 and rows[0][3:5] == ("ns/a", "ingress") and rows[0][7:] == ("2022-03-06", 90)
        mean, std, _ = dro.drop_detection_series(num[:12])
        assert rows[0][5] == mean and rows[0][6] == std
    finally:
        ad.set_engine(None)
