"""GPU, end to end: a StreamingAnomalyDetection fed by overlapping re-read polls (feed(flows, replace=(from_t, to_t)) and poll())
answers its jobs as anomaly_detection() does over the table with every row ONCE.  About 5000 seeded rows over 60 minute steps arrive up
to three steps late; eight polls each re-read everything that has arrived in [watermark - lag, now).  Every row is read two or three
times; the default feed would double or triple its throughput under the modes' sum.  Half-way the instance is snapshotted, closed and
restored, watermark included."""

import numpy as np
import pytest

from theia_amd import anomaly_detection as ad
from theia_amd import clickhouse as ch
from theia_amd.stream_detection import StreamingAnomalyDetection
from stream_helpers import IGNORE, LAG, MODES, STEP, T0, TableClient, comparable, replace_table, turns  # noqa: F401  (replace_table: the fixture `table`)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,ident", MODES, ids=["svc", "pod-labels", "pod-name"])
def test_overlapping_replace_polls_answer_like_the_batch_job_over_each_row_once(engine, table, mode, ident):
    flows, arrival = table
    client = TableClient(flows, arrival)
    s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
    replaced = 0
    for p, now in enumerate(turns()):
        client.now = now
        if p == 4:      # a restart between two turns: the watermark comes back with the state
            snap = s.snapshot()
            wm = s.watermark
            s.close()
            s = StreamingAnomalyDetection.restore(engine, snap, mode, pod_ident=ident, ns_ignore_list=IGNORE)
            assert s.watermark == wm == turns()[3]
        if p % 2:       # the loop by hand: the same read, fed with replace
            from_t = max(s.watermark - LAG, 0)
            got = client.query_columns(ch.stream_rows_query(mode, ident, list(IGNORE), from_t, now))
            stats = s.feed(got, replace=(from_t, now))
            s.watermark = now
        else:
            stats = s.poll(client, now, LAG)
        assert s.watermark == now
        replaced += stats["points_replaced"]
        assert p == 0 or stats["points_replaced"] > 0, (p, stats)
    # the polls did overlap (svc: 6 keys x 4 steps of lag x 7 later turns is at most 168 points): under the default feed these would have doubled
    assert replaced > 100
    assert ("toDateTime(%d)" % (turns()[3] - LAG)) in client.queries[4]
    filters = {"svc": [dict(), dict(svc_port_name="shop/web:http")], "labels": [dict(), dict(pod_label="web")],
               "name": [dict(pod_name="web-0"), dict(pod_name="db-0", pod_namespace="shop")]}[mode if mode == "svc" else ident]
    real = 0
    for algo in ("EWMA", "DBSCAN"):
        for filt in filters:
            _, want = ad.anomaly_detection(algo, flows, "", "", "job-1", IGNORE, mode, engine=engine, **filt)
            _, got = s.job(algo, "job-1", **filt)
            assert comparable(got, s.mode) == comparable(want, s.mode), (mode, ident, algo, filt)
            real += want[0]["anomaly"] == "true"
    assert real >= 2
    # a turn made again (a retry after a timeout) changes nothing, and a re-read that finds no row erases its seconds
    before = s.state.export_series()
    s.watermark = turns()[6]
    s.poll(client, turns()[7], LAG)
    assert np.array_equal(s.state.export_series()[1], before[1])
    empty = {c: flows[c][:0] for c in flows}
    st = s.feed(empty, replace=(T0, T0 + 10 * STEP))
    assert st["points_erased"] > 0 and st["batch_points"] == 0
    assert int(s.state.export_times().min()) >= T0 + 10 * STEP
    s.close()


def test_the_default_feed_doubles_what_the_polls_read_twice(engine, table):
    """the fault the replace form is for, on the same reads"""
    flows, arrival = table
    client = TableClient(flows, arrival)
    a = StreamingAnomalyDetection(engine, "svc", ns_ignore_list=IGNORE)
    b = StreamingAnomalyDetection(engine, "svc", ns_ignore_list=IGNORE)
    wm = 0
    for now in turns():
        client.now = now
        from_t = max(wm - LAG, 0)
        got = client.query_columns(ch.stream_rows_query("svc", "labels", list(IGNORE), from_t, now))
        a.feed(got, replace=(from_t, now))
        b.feed(got)
        wm = now
    assert np.array_equal(a.state.export_times(), b.state.export_times())
    va, vb = a.state.export_series()[1], b.state.export_series()[1]
    assert (vb >= va).all() and (vb > va).sum() > 100
    a.close()
    b.close()
