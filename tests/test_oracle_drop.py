"""The drop-detection oracle (oracle/drop_oracle.py) pinned against the REFERENCE UDF: its own golden test
(snowflake/udfs/udfs/drop_detection/drop_detection_udf_test.py:130-139) and outputs of the reference code run on
seeded series in the build container (tests/golden/drop_outputs.json, made by oracle/make_golden.py)."""
import json
import os

import numpy as np
import pytest

from oracle import drop_oracle as dro
from oracle import tad_oracle as orc

import drop_tables as dt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drop_outputs.json")


@pytest.fixture(scope="module")
def drop_golden():
    with open(GOLD) as f:
        return json.load(f)


def test_reference_unit_test_golden(drop_golden):
    x = drop_golden["series"]["reference_test"]["x"]
    mean, std, verdict = dro.drop_detection_series(x)
    # drop_detection_udf_test.py asserts exact equality on these
    assert [["antrea-test/Pod-A", "ingress", mean, std, "2022-01-05", 100]] == drop_golden["expected_result"]
    assert np.flatnonzero(verdict).tolist() == [4]


def test_oracle_equals_reference_udf_outputs_bit_for_bit(drop_golden):
    for name, e in drop_golden["series"].items():
        r = dro.drop_detection_series(e["x"])
        if len(e["x"]) < 3:
            assert r is None and e["rows"] == [], name
            continue
        mean, std, verdict = r
        want_idx = [int(row[2].split("-")[1]) for row in e["rows"]]
        assert np.flatnonzero(verdict).tolist() == want_idx, name
        for row in e["rows"]:
            assert row[0] == mean and row[1] == std, (name, row[:2], mean, std)     # exact: same summation order as numpy
            assert row[3] == e["x"][int(row[2].split("-")[1])]


def test_pairwise_sum_is_numpy_sum():
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 127, 128, 129, 1000, 4099):
        a = rng.normal(0, 1e9, size=n)
        assert dro.pairwise_sum(a) == float(np.add.reduce(a))


def test_pairwise_sum_is_numpy_sum_at_every_length_of_the_gpu_boundary_tests():
    """tests/test_gpu_drop_boundaries.py holds the kernel to the oracle at every length 1 .. 300, 511 .. 529, 1023 .. 1041, 2049 and 4100
    (its other tables' lengths lie within 1 .. 300): there the oracle's sum, and the vectorised mirror the tables are drawn with, must
    be numpy's add-reduce — on values and on squared deviations whose sums depend on the order (drop_tables.order_sensitive)."""
    rng = np.random.default_rng(6)
    for n in dt.ALL_LENGTHS:
        for dip in (False, True):
            x = orc.u64_to_f64(dt.draw_key(rng, n, dip))
            assert n < 4 or dt.order_sensitive(x), n
            sq = (dro.drop_stats(x)[0] - x) ** 2 if n >= 2 else x
            for a in (x, sq):
                assert dro.pairwise_sum(a) == float(np.add.reduce(a)), n
            both = np.stack([x, sq])
            assert dt.pairwise_rows(both).tolist() == [dro.pairwise_sum(x), dro.pairwise_sum(sq)], n
            if n >= 4:
                assert bool(dt.order_sensitive_rows(x[None, :])[0]) == dt.order_sensitive(x), n
    a = np.array([2.0**53, 1.0, 1.0, 2.0**53, 1.0, 1.0, 1.0])        # the tree of eight on a zero-padded series is not the left-to-right sum
    assert dt.tree_of_eight_rows(a[None, :])[0] == 2.0**54 + 4 and dro.pairwise_sum(a) == 2.0**54


def test_boundary_tables_are_order_sensitive_and_laid_out_as_described():
    """the conditions tests/test_gpu_drop_boundaries.py asserts before it asks the engine hold on the host: at least two order-sensitive
    keys of every length >= 4, half the keys contiguous and half with missing days"""
    for tab, lengths, per in ((dt.short_table(), dt.SHORT_LENGTHS, 4), (dt.long_table(), dt.LONG_LENGTHS, 2)):
        dt.assert_order_sensitive(tab, lengths)
        dt.assert_days_layout(tab)
        assert tab.K == per * len(lengths) and np.bincount(tab.lengths).tolist() == np.bincount(np.repeat(lengths, per)).tolist()
        assert int(tab.v.max()) < 2**53 and np.unique(np.stack([tab.key, tab.t.astype(np.uint64)]), axis=1).shape[1] == tab.key.size      # one row per point


def test_a_result_needs_min_samples_and_two_points():
    """include/tad.h: a key has a result iff n >= drop_min_samples and n >= 2"""
    one, two = [5], [5, 9]
    for ms in (1, 2, 3):
        assert dro.drop_detection_series(one, min_samples=ms) is None
        assert (dro.drop_detection_series(two, min_samples=ms) is None) == (ms == 3)
    mean, std, verdict = dro.drop_detection_series(two, min_samples=1)
    assert (mean, std) == (7.0, float(np.sqrt(8.0))) and not verdict.any()
    assert dro.drop_detection_series([], min_samples=1) is None
    key = np.array([0, 1, 1, 2, 2, 2], dtype=np.uint64)
    day = np.array([0, 0, 1, 0, 1, 2], dtype=np.int64)
    val = np.array([5, 5, 9, 1, 2, 90], dtype=np.uint64)
    for ms, skipped in ((1, 1), (2, 1), (3, 2), (4, 3)):
        job = dro.run_job(key, day, val, n_sigma=0.5, min_samples=ms)
        assert job["keys_no_result"] == skipped and job["n_keys"] == 3 and job["n_points"] == 6, ms
        assert set(job["key_id"].tolist()) == ({1, 2} if ms <= 2 else {2} if ms == 3 else set())


def test_run_job_passes_the_stage0_arguments_through():
    rng = np.random.default_rng(8)
    n, K = 4000, 40
    key = rng.integers(0, K, size=n).astype(np.uint64)
    key2 = np.where(rng.random(n) < 0.3, orc.KEY_SKIP, rng.integers(0, K, size=n).astype(np.uint64))
    key = np.where(rng.random(n) < 0.1, orc.KEY_SKIP, key)
    day = 19000 + rng.integers(0, 30, size=n).astype(np.int64)
    start = day - rng.integers(0, 3, size=n)
    val = rng.integers(1 << 52, 1 << 53, size=n, dtype=np.uint64)
    seen = []
    for kw in (dict(value_op="max"), dict(key_id2=key2), dict(flow_start_s=start, start_time=19004), dict(end_time=19020),
               dict(value_op="max", key_id2=key2, flow_start_s=start, start_time=19003, end_time=19025), {}):
        job = dro.run_job(key, day, val, n_sigma=1.5, min_samples=4, **kw)
        pk, pt, pv = orc.stage0(key, day, val, kw.get("value_op", "sum"), kw.get("key_id2"), kw.get("flow_start_s"), kw.get("start_time", 0),
                                kw.get("end_time", 0))
        keys, ptr = orc.series_offsets(pk)
        x = orc.u64_to_f64(pv)
        rows, skipped = [], 0
        for a, b in zip(ptr[:-1], ptr[1:]):
            r = dro.drop_detection_series(x[a:b], 1.5, 4)
            skipped += r is None
            if r is not None:
                rows += [(int(pk[i]), int(pt[i]), x[i], r[0], r[1]) for i in a + np.flatnonzero(r[2])]
        got = list(zip(job["key_id"].tolist(), job["flow_end_s"].tolist(), job["throughput"].tolist(), job["algo_calc"].tolist(), job["stddev"].tolist()))
        assert got == rows and len(rows) > 0, kw
        assert (job["n_points"], job["n_keys"], job["keys_no_result"], job["n_anomalies"]) == (pk.size, keys.size, skipped, len(rows)), kw
        seen.append((job["n_points"], job["n_anomalies"], float(x.sum())))
    assert len(set(seen)) == len(seen)                      # every argument changed the job


def test_against_the_live_reference_udf(drop_golden):
    """The reference UDF's rows on these seeded series, recorded by oracle/make_golden.py running it (tests/golden/drop_outputs.json,
    `live_udf`): the oracle must give the same anomalous days and the same mean / std bits."""
    rng = np.random.default_rng(9)
    recorded = drop_golden["live_udf"]
    assert len(recorded) == 4
    for n, e in zip((3, 50, 200, 600), recorded):
        x = rng.poisson(20.0, size=n).astype(np.int64)
        x[rng.integers(0, n)] *= 40
        assert x.tolist() == e["x"], n
        rows = e["rows"]
        mean, std, verdict = dro.drop_detection_series(x)
        assert [r[2] for r in rows] == np.flatnonzero(verdict).tolist()
        assert all(r[0] == mean and r[1] == std for r in rows)
