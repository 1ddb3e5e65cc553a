"""GPU: StreamingAnomalyDetection judged in time buckets (job / feed_alerts / poll_alerts with bucket_s; TadEngine.run_state_buckets under
them).  An instance is fed SECOND-resolution flow rows in shuffled batches; job(bucket_s=60) must return, row for row, what
anomaly_detection() returns over the same rows with flowEndSeconds floored to the minute — a name filter, an end_time and complete_before
included.  poll_alerts(bucket_s=60) runs through the ClickHouse stand-in of tests/test_gpu_stream_replace.py over overlapping re-reads: its
rows are job(bucket_s=60)'s restricted to the buckets from each changed key's first changed bucket on, and the same turn made twice returns
nothing."""
import time

import numpy as np
import pytest

from theia_amd import anomaly_detection as ad
from theia_amd.stream_detection import StreamingAnomalyDetection
from stream_helpers import BUCKET, IGNORE, SPAN, T0, TableClient, batches, changed_since, comparable, held, key_tuples, seconds_table  # noqa: F401  (seconds_table: the fixture `table`)

pytestmark = pytest.mark.gpu

MODES = [("svc", "labels"), ("pod", "labels")]
FILTERS = {"svc": [dict(svc_port_name="shop/web:http"), dict()], "pod": [dict(pod_label="web"), dict()]}


def floored(flows, before=None):
    """the rows with flowEndSeconds floored to the bucket (and only those that end before `before`)"""
    t = flows["flowEndSeconds"]
    sel = np.ones(t.size, bool) if before is None else t < before
    out = {c: v[sel] for c, v in flows.items()}
    out["flowEndSeconds"] = (out["flowEndSeconds"] // BUCKET) * BUCKET
    return out


def stamp(t):
    return time.strftime(ad.TIME_FORMAT, time.gmtime(t))


@pytest.mark.parametrize("mode,ident", MODES, ids=["svc", "pod"])
def test_a_bucketed_job_is_the_batch_job_over_the_floored_rows(engine, table, mode, ident):
    flows, _ = table
    s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
    for b in batches(flows):
        s.feed(b)
    raw_points = s.state.series_points()
    real = 0
    end = ((T0 + 45 * 60) // BUCKET) * BUCKET
    now = T0 + 50 * 60 + 17                                    # inside a minute: complete_before ends the window at that minute's start
    for algo in ("EWMA", "DBSCAN", "ARIMA"):
        for filt in FILTERS[mode]:
            _, want = ad.anomaly_detection(algo, floored(flows), "", "", "job-1", IGNORE, mode, engine=engine, **filt)
            stats, got = s.job(algo, "job-1", bucket_s=BUCKET, **filt)
            assert comparable(got, s.mode) == comparable(want, s.mode), (mode, algo, filt, len(got), len(want))
            assert all(r["flowEndSeconds"] % BUCKET == 0 for r in got if r["anomaly"] == "true")
            real += want[0]["anomaly"] == "true"
            if not filt:
                assert stats["rows_in"] == raw_points > stats["n_points"] > 0, (stats["rows_in"], raw_points, stats["n_points"])
        if mode == "svc":                                      # end_time bounds flowEndSeconds (the pod query has no time filter)
            _, want = ad.anomaly_detection(algo, floored(flows), "", stamp(end), "job-1", IGNORE, mode, engine=engine)
            _, got = s.job(algo, "job-1", end_time=stamp(end), bucket_s=BUCKET)
            assert comparable(got, s.mode) == comparable(want, s.mode), (mode, algo, "end_time")
        _, want = ad.anomaly_detection(algo, floored(flows, before=(now // BUCKET) * BUCKET), "", "", "job-1", IGNORE, mode, engine=engine)
        _, got = s.job(algo, "job-1", bucket_s=BUCKET, complete_before=now)
        assert comparable(got, s.mode) == comparable(want, s.mode), (mode, algo, "complete_before")
        assert max(r["flowEndSeconds"] for r in got) < (now // BUCKET) * BUCKET
    assert real >= 3
    # bucket_s = 0 is the job as it was; what the bucketed job refuses
    _, want = ad.anomaly_detection("EWMA", flows, "", "", "job-1", IGNORE, mode, engine=engine)
    assert comparable(s.job("EWMA", "job-1")[1], s.mode) == comparable(want, s.mode)
    assert comparable(s.job("EWMA", "job-1", bucket_s=0, bucket_op="sum")[1], s.mode) == comparable(want, s.mode)
    if mode == "svc":
        with pytest.raises(ValueError):
            s.job("EWMA", "job-1", end_time=stamp(end + 7), bucket_s=BUCKET)
    for bad in (dict(bucket_s=-1), dict(bucket_s=BUCKET, bucket_op="avg"), dict(complete_before=now)):
        with pytest.raises(ValueError):
            s.job("EWMA", "job-1", **bad)
    s.close()


def expected_alerts(s, algo, filt, since):
    """job(bucket_s)'s anomalous rows of the changed keys from the bucket that holds their first changed second on; no sentinel"""
    tuples = key_tuples(s)
    by_tuple = {tuples[k]: (t // BUCKET) * BUCKET for k, t in since.items()}
    _, rows = s.job(algo, "job-1", bucket_s=BUCKET, **filt)
    names = ad.KEY_COLUMNS[s.mode]
    out = []
    for r in rows:
        if r["anomaly"] != "true":
            continue
        t = by_tuple.get(tuple(str(r[c]) for c in names))
        if t is not None and r["flowEndSeconds"] >= t:
            out.append(r)
    return out


@pytest.mark.parametrize("mode,ident", MODES, ids=["svc", "pod"])
def test_bucketed_alert_turns_report_from_each_changed_keys_first_changed_bucket_on(engine, table, mode, ident):
    flows, arrival = table
    client = TableClient(flows, arrival)
    s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
    lag = 240
    nows = [T0 + 450 * (p + 1) + 11 for p in range(8)] + [T0 + SPAN + 200]
    reported = inside = 0
    for p, now in enumerate(nows):
        client.now = now
        algo = ("EWMA", "DBSCAN")[p % 2]
        filt = FILTERS[mode][p % 2]
        before = held(s)
        stats, rows = s.poll_alerts(client, now, lag, algo, "job-1", bucket_s=BUCKET, **filt)
        since = changed_since(before, held(s))
        assert stats["keys_changed"] == len(since) > 0, (p, stats)
        inside += sum(1 for t in since.values() if t % BUCKET)
        want = expected_alerts(s, algo, filt, since)
        assert comparable(rows, s.mode) == comparable(want, s.mode), (mode, p, algo, filt, len(rows), len(want))
        assert all(r["anomaly"] == "true" and r["flowEndSeconds"] % BUCKET == 0 for r in rows)
        reported += len(rows)
    assert reported >= 2 and inside >= 2                        # rows were reported, and first changed seconds lay inside a minute
    # the same turn made twice returns nothing
    s.watermark = nows[-2]
    stats, rows = s.poll_alerts(client, nows[-1], lag, "EWMA", "job-1", bucket_s=BUCKET)
    assert rows == [] and stats["keys_changed"] == 0 and stats["points_replaced"] > 0
    s.close()
