"""GPU: StreamingAnomalyDetection.rollup — retention on a long-lived instance (TadState.rollup under it).  Two instances are fed the same
second-resolution rows (the table of tests/test_gpu_stream_buckets.py); one rolls everything older than a bound into minutes.  Its
job(bucket_s=...) at the minute and at a multiple of it returns, row for row, what the instance that never rolled up returns; what the
rolled region cannot answer is refused (a job below its resolution or with another operation, a re-read that starts inside a bucket) and
`poll` floors its re-read's start instead; snapshot / restore carry the tiers; over twenty feed-and-rollup rounds the device bytes stay
bounded while an instance without retention grows."""
import re

import numpy as np
import pytest

from theia_amd.stream_detection import StreamingAnomalyDetection
from state_helpers import assert_same, snapshot
from stream_helpers import BUCKET, IGNORE, SPAN, SVCS, T0, TableClient, batches, comparable, seconds_table  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

BOUND = ((T0 + 40 * 60) // BUCKET) * BUCKET


def fed(engine, flows, mode="svc", ident="labels"):
    s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
    for b in batches(flows):
        s.feed(b)
    return s


@pytest.mark.parametrize("mode,ident", [("svc", "labels"), ("pod", "labels")], ids=["svc", "pod"])
def test_jobs_at_the_rolled_resolution_equal_those_of_an_instance_that_never_rolled_up(engine, table, mode, ident):
    flows, _ = table
    a, b = fed(engine, flows, mode, ident), fed(engine, flows, mode, ident)
    points, nbytes = a.state.series_points(), a.device_bytes()
    stats = a.rollup(BOUND + 17, BUCKET)
    assert stats["before_t"] == BOUND and a.tiers == [(BOUND, BUCKET, "sum")]
    assert stats["points_before"] == points and a.state.series_points() == stats["points_after"] < points * 2 // 3
    assert a.device_bytes() <= nbytes
    real = 0
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        for bucket_s in (BUCKET, 5 * BUCKET):
            sa, got = a.job(algo, "job-1", bucket_s=bucket_s)
            sb, want = b.job(algo, "job-1", bucket_s=bucket_s)
            assert comparable(got, a.mode) == comparable(want, b.mode), (mode, algo, bucket_s, len(got), len(want))
            assert sa["n_points"] == sb["n_points"] and sa["rows_in"] < sb["rows_in"]
            real += want[0]["anomaly"] == "true"
        _, got = a.job(algo, "job-1", bucket_s=BUCKET, complete_before=T0 + 50 * 60 + 17)
        _, want = b.job(algo, "job-1", bucket_s=BUCKET, complete_before=T0 + 50 * 60 + 17)
        assert comparable(got, a.mode) == comparable(want, b.mode), (mode, algo, "complete_before")
    assert real >= 2
    # the same roll-up again: one tier, nothing changes; a further one at the same resolution moves the tier's bound
    snap = snapshot(a.state)
    assert a.rollup(BOUND, BUCKET)["keys_changed"] == 0 and a.tiers == [(BOUND, BUCKET, "sum")]
    assert_same(snapshot(a.state), snap, "idempotent")
    a.rollup(BOUND + 300, BUCKET)
    assert a.tiers == [(BOUND + 300, BUCKET, "sum")]
    _, got = a.job("EWMA", "job-1", bucket_s=BUCKET)
    _, want = b.job("EWMA", "job-1", bucket_s=BUCKET)
    assert comparable(got, a.mode) == comparable(want, b.mode)
    a.close(), b.close()


def test_the_guards_of_an_instance_that_rolled_up(engine, table):
    flows, arrival = table
    a, b = fed(engine, flows), fed(engine, flows)
    assert b.rollup(BOUND, BUCKET, "sum")["points_after"] > 0
    # 1. a job that reaches the rolled region below its resolution, off its multiples or with another operation
    for bad in (dict(), dict(bucket_s=0), dict(bucket_s=90), dict(bucket_s=30), dict(bucket_s=BUCKET, bucket_op="max")):
        with pytest.raises(ValueError) as ei:
            b.job("EWMA", "job-1", **bad)
        assert "rolled up" in str(ei.value), bad
        a.job("EWMA", "job-1", **bad)                             # an instance that never rolled up answers all of them
    with pytest.raises(ValueError):
        b.feed_alerts({c: v[:0] for c, v in flows.items()}, "EWMA", "job-1")
    # 2. a re-read that starts inside a bucket of the rolled region
    t = flows["flowEndSeconds"]
    snap = snapshot(b.state)
    inside = BOUND - 5 * BUCKET + 7
    sel = (t >= inside) & (t < BOUND + 600)
    with pytest.raises(ValueError) as ei:
        b.feed({c: v[sel] for c, v in flows.items()}, replace=(inside, BOUND + 600))
    assert "bucket start" in str(ei.value)
    assert_same(snapshot(b.state), snap, "a refused re-read")
    a.feed({c: v[sel] for c, v in flows.items()}, replace=(inside, BOUND + 600))       # no tier: as before
    start = inside // BUCKET * BUCKET
    sel = (t >= start) & (t < BOUND + 600)
    assert b.feed({c: v[sel] for c, v in flows.items()}, replace=(start, BOUND + 600))["points_replaced"] > 0
    sel = (t >= BOUND + 7) & (t < BOUND + 600)                    # at or after the bound: any second
    b.feed({c: v[sel] for c, v in flows.items()}, replace=(BOUND + 7, BOUND + 600))
    sel = t < BOUND + 600                                         # no lower bound: everything is re-read
    b.feed({c: v[sel] for c, v in flows.items()}, replace=(0, BOUND + 600))
    _, got = b.job("EWMA", "job-1", bucket_s=BUCKET)
    _, want = a.job("EWMA", "job-1", bucket_s=BUCKET)
    assert comparable(got, b.mode) == comparable(want, a.mode)
    # 3. poll floors its re-read's start to the tier's bucket start
    b.rollup(BOUND, BUCKET)
    client = TableClient(flows, arrival)
    client.now = T0 + SPAN + 1000                                 # every row has arrived
    b.watermark = inside + 240
    b.poll(client, T0 + SPAN + 1, 240)
    assert int(re.search(r"flowEndSeconds >= toDateTime\((\d+)\)", client.queries[-1]).group(1)) == start != inside
    a.watermark = inside + 240
    a.poll(client, T0 + SPAN + 1, 240)
    assert int(re.search(r"flowEndSeconds >= toDateTime\((\d+)\)", client.queries[-1]).group(1)) == inside
    _, got = b.job("DBSCAN", "job-1", bucket_s=BUCKET)
    _, want = a.job("DBSCAN", "job-1", bucket_s=BUCKET)
    assert comparable(got, b.mode) == comparable(want, a.mode)
    a.close(), b.close()


def test_snapshot_and_restore_carry_the_tiers(engine, table):
    flows, _ = table
    a = fed(engine, flows)
    plain = a.snapshot()
    assert "rollup_tiers" not in plain                            # an instance that never rolled up snapshots what it always did
    a.rollup(BOUND - 1200, 300, "sum"), a.rollup(BOUND, BUCKET, "sum")
    assert a.tiers == [(BOUND - 1200 - (BOUND - 1200) % 300, 300, "sum"), (BOUND, BUCKET, "sum")]
    snap = a.snapshot()
    b = StreamingAnomalyDetection.restore(engine, snap, "svc", ns_ignore_list=IGNORE)
    assert b.tiers == a.tiers
    assert_same(snapshot(b.state), snapshot(a.state), "restored")
    with pytest.raises(ValueError):
        b.job("EWMA", "job-1", bucket_s=BUCKET)                   # reaches the 300 s tier
    _, got = b.job("EWMA", "job-1", bucket_s=300)
    _, want = a.job("EWMA", "job-1", bucket_s=300)
    assert comparable(got, b.mode) == comparable(want, a.mode)
    # a snapshot without tiers (of before the roll-up existed, or of an instance that never rolled up) restores as it always did
    c = StreamingAnomalyDetection.restore(engine, plain, "svc", ns_ignore_list=IGNORE)
    assert c.tiers == [] and c.job("EWMA", "job-1")[1]
    old = {k: v for k, v in snap.items() if k != "rollup_tiers"}
    d = StreamingAnomalyDetection.restore(engine, old, "svc", ns_ignore_list=IGNORE)
    assert d.tiers == [] and d.state.series_points() == a.state.series_points()
    for s in (a, b, c, d):
        s.close()


def test_device_bytes_stay_bounded_over_twenty_feed_and_rollup_rounds(engine):
    rng = np.random.default_rng(77)
    svcs = [s for s in SVCS if s]
    a = StreamingAnomalyDetection(engine, "svc")
    b = StreamingAnomalyDetection(engine, "svc")
    ROUND, KEEP = 600, 900                                        # ten minutes of seconds per round; the newest fifteen stay at full resolution
    t0 = (T0 // BUCKET) * BUCKET
    sizes_a, sizes_b, points = [], [], []
    for r in range(20):
        sec = np.repeat(np.arange(r * ROUND, (r + 1) * ROUND), len(svcs))
        n = sec.size
        flows = {"sourcePodNamespace": np.full(n, "shop"), "destinationPodNamespace": np.full(n, "shop"),
                 "destinationServicePortName": np.tile(np.array(svcs), ROUND), "flowType": np.ones(n, np.int64),
                 "flowEndSeconds": (t0 + sec).astype(np.int64), "flowStartSeconds": (t0 + sec - 30).astype(np.int64),
                 "throughput": rng.integers(1_000_000, 9_000_000, n).astype(np.uint64)}
        a.feed(flows), b.feed(flows)
        a.rollup(t0 + (r + 1) * ROUND - KEEP, BUCKET)
        sizes_a.append(a.device_bytes()), sizes_b.append(b.device_bytes()), points.append(a.state.series_points())
        assert points[-1] <= len(svcs) * ((r + 1) * ROUND // BUCKET + KEEP + BUCKET), (r, points[-1])
    assert points[-1] < b.state.series_points() // 8
    assert max(sizes_a[10:]) <= 2 * max(sizes_a[:10]), (sizes_a,)              # bounded: no round of the second half needs twice the first half's
    assert b.state.nbytes() > 2 * a.state.nbytes(), (b.state.nbytes(), a.state.nbytes(), sizes_a, sizes_b)   # ... where the instance without retention kept growing
    _, got = a.job("EWMA", "job-1", bucket_s=BUCKET)
    _, want = b.job("EWMA", "job-1", bucket_s=BUCKET)
    assert comparable(got, a.mode) == comparable(want, b.mode)
    a.close(), b.close()
