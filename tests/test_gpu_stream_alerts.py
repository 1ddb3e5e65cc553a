"""GPU, end to end: the alert feed of a StreamingAnomalyDetection (feed_alerts / poll_alerts) and the periodical drop job's partial days.

feed_alerts / poll_alerts against `job`: after every turn the rows must be exactly `job`'s rows (same filters, over everything held)
restricted to the keys the turn changed, from each key's first changed time on.  Which keys changed, and from when, is read off the
state's exports before and after the turn, on the host — not from the report under test.  The polls re-read a lag through the in-process
ClickHouse stand-in of tests/test_gpu_stream_replace.py, so most turns replace points by their own value, which must not count as change.

The drop job, twice.  Flow rows (feed_flows): the 40 endpoints x 20 days flow table of tests/test_gpu_drop_select.py, every day's rows cut
over three partial feeds; counts (feed): a table of 40 endpoints x 20 days of daily counts cut so that every day arrives in two or three
partial feeds.  Each feed is compared with oracle/drop_oracle.py on the cumulative counts, restricted to the changed partitions and
days; at the end window() is the batch job over the whole table, and the default feed still refuses a split day."""
import numpy as np
import pytest

from oracle import drop_oracle as dro
from theia_amd import TadError
from theia_amd import anomaly_detection as ad
from theia_amd.drop_detection import PeriodicalDropDetection, drop_detection_table
from theia_amd.stream_detection import StreamingAnomalyDetection

import drop_query_ref as dq
from stream_helpers import (DAY0, IGNORE, LAG, MODES, N_DAYS, STEP, T0, TableClient, changed_since, comparable, counts_of, flows, held, key_tuples,
                            keyed, replace_table, turns)  # noqa: F401  (table: the module's fixture)

pytestmark = pytest.mark.gpu

FILTERS = {("svc", "labels"): dict(svc_port_name="shop/web:http"), ("pod", "labels"): dict(pod_label="web"), ("pod", "name"): dict(pod_name="web-0")}


def expected_alerts(s, algo, filt, since):
    """job's rows of the changed keys from their first changed time on; no sentinel"""
    tuples = key_tuples(s)
    by_tuple = {tuples[k]: t for k, t in since.items()}
    _, rows = s.job(algo, "job-1", **filt)
    names = ad.KEY_COLUMNS[s.mode]
    out = []
    for r in rows:
        if r["anomaly"] != "true":
            continue
        t = by_tuple.get(tuple(str(r[c]) for c in names))
        if t is not None and r["flowEndSeconds"] >= t:
            out.append(r)
    return out


@pytest.mark.parametrize("mode,ident", MODES, ids=["svc", "pod-labels", "pod-name"])
def test_alert_turns_report_jobs_rows_of_the_changed_keys_from_their_changed_time_on(engine, table, mode, ident):  # noqa: F811
    flows, arrival = table
    client = TableClient(flows, arrival)
    s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
    reported = unchanged_replaced = 0
    base = dict(pod_name="db-0", pod_namespace="shop") if ident == "name" else {}      # (a by-name instance serves jobs with a pod_name only)
    any_web0 = dict(pod_name="web-0") if ident == "name" else {}
    for p, now in enumerate(turns()):
        client.now = now
        algo = ("EWMA", "DBSCAN")[p % 2]
        filt = base if p % 3 == 0 else FILTERS[(mode, ident)]
        before = held(s)
        stats, rows = s.poll_alerts(client, now, LAG, algo, "job-1", **filt)
        since = changed_since(before, held(s))
        assert s.watermark == now and "key_since" not in stats
        assert stats["keys_changed"] == len(since) and stats["keys_changed"] <= stats["keys_touched"], (p, stats, len(since))
        assert since and stats["min_t"] == min(since.values()) and stats["points_changed"] >= len(since), (p, stats)
        unchanged_replaced += stats["points_replaced"] + stats["points_appended"] + stats["points_inserted"] + stats["points_erased"] - stats["points_changed"]
        want = expected_alerts(s, algo, filt, since)
        assert comparable(rows, s.mode) == comparable(want, s.mode), (mode, ident, p, algo, filt, len(rows), len(want))
        assert all(r["anomaly"] == "true" for r in rows)
        reported += len(rows)
    assert reported >= 2 and unchanged_replaced > 50          # rows were reported, and most re-read points were replaced by their own value
    # the same turn made twice: the state and the alerts are idempotent
    s.watermark = turns()[6]
    stats, rows = s.poll_alerts(client, turns()[7], LAG, "EWMA", "job-1", **any_web0)
    assert rows == [] and stats["keys_changed"] == 0 and stats["points_changed"] == 0 and stats["points_replaced"] > 0
    # a late row for one key reports only that key, from its time on
    before = held(s)
    one = {c: flows[c][:0] for c in flows}
    if mode == "svc":
        late = dict(one, destinationServicePortName=np.array(["shop/db:pg"]), flowType=np.array([1]), sourcePodNamespace=np.array(["shop"]),
                    destinationPodNamespace=np.array(["shop"]))
    else:
        late = dict(one, sourcePodNamespace=np.array([""]), sourcePodName=np.array([""]), sourcePodLabels=np.array([""]),
                    destinationPodNamespace=np.array(["shop"]), destinationPodName=np.array(["web-0"]),
                    destinationPodLabels=np.array(['{"app":"web","pod-template-hash":"h0","tier":"t0"}']), flowType=np.array([1]))
    for c in late:
        if late[c].size == 0:
            late[c] = np.array([""]) if flows[c].dtype.kind in "US" else np.zeros(1, flows[c].dtype)
    late["flowEndSeconds"] = np.array([T0 + 30 * STEP], np.int64)
    late["throughput"] = np.array([90_000_000_000], np.uint64)
    stats, rows = s.feed_alerts(late, "EWMA", "job-1", **any_web0)
    since = changed_since(before, held(s))
    assert list(since.values()) == [T0 + 30 * STEP] and stats["keys_changed"] == 1 and stats["points_changed"] == 1, (since, stats)
    assert comparable(rows, s.mode) == comparable(expected_alerts(s, "EWMA", any_web0, since), s.mode)
    assert rows and all(r["flowEndSeconds"] >= T0 + 30 * STEP for r in rows) and len({tuple(r[c] for c in ad.KEY_COLUMNS[s.mode]) for r in rows}) == 1
    # what the instance does not serve is refused before the feed changes anything
    before = held(s)
    with pytest.raises(ValueError):
        s.feed_alerts(late, "NOPE", "job-1", **any_web0)
    if mode == "pod":
        with pytest.raises(ValueError):
            s.feed_alerts(late, "EWMA", "job-1", **({"pod_name": "x"} if ident == "labels" else {"pod_label": "x"}))
    assert held(s) == before
    s.close()


def drop_table():
    """40 endpoints x 20 days, in (endpoint, day) order: (endpoint, direction, day numbers, counts)"""
    rng = np.random.default_rng(40)
    n_ep, n_day = 40, 20
    ep = np.repeat(np.array(["ns%d/pod-%d" % (i % 4, i) for i in range(n_ep)]), n_day)
    di = np.repeat(np.array(["ingress", "egress"])[np.arange(n_ep) % 2], n_day)
    day = np.tile(19000 + np.arange(n_day, dtype=np.int64), n_ep)
    cnt = rng.integers(40, 60, size=n_ep * n_day).astype(np.uint64)
    spikes = rng.random(cnt.size) < 0.06
    cnt[spikes] = cnt[spikes] * 9
    return ep, di, day, cnt


def drop_oracle(ep, di, day, cnt, report):
    """the anomalous (endpoint, day) of the cumulative counts among the points `report` names: {(endpoint, day): (count, mean, std)}"""
    out = {}
    for e in np.unique(ep):
        m = ep == e
        o = np.argsort(day[m])
        d, x = day[m][o], cnt[m][o].astype(np.float64)
        r = dro.drop_detection_series(x, 3.0, 3) if x.size >= 2 else None
        if r is None:
            continue
        mean, std, z = r
        for i in np.flatnonzero(z):
            if report(e, int(d[i])):
                out[(str(e), int(d[i]))] = (int(x[i]), float(mean), float(std))
    return out


def rows_map(rows):
    return {(r[3], int(r[7])): (r[8], r[5], r[6]) for r in rows}


def test_the_drop_job_takes_a_day_in_two_or_three_partial_feeds(engine):
    ep, di, day, cnt = drop_table()
    rng = np.random.default_rng(41)
    job = PeriodicalDropDetection(engine)
    got_ep, got_day, got_cnt = np.zeros(0, ep.dtype), np.zeros(0, np.int64), np.zeros(0, np.uint64)
    feeds = 0
    for d0 in range(19000, 19020, 4):                         # four days at a time, each day's counts cut into two or three parts
        block = (day >= d0) & (day < d0 + 4)
        parts = np.where(rng.random(cnt.size) < 0.5, 2, 3)
        for part in range(3):
            sel = block & (part < parts)
            share = np.where(part == parts - 1, cnt - (cnt // parts) * (parts - 1), cnt // parts).astype(np.uint64)
            if part == 1:                                      # the second feed of a block leaves every third endpoint out
                sel &= ~np.isin(np.array([e[-1] for e in ep.tolist()]), list("0369"))
                held_back = block & (part < parts) & ~sel
            o = rng.permutation(np.flatnonzero(sel))
            rows = job.feed(ep[o], di[o], day[o], share[o], detection_id="d", partial=True)
            feeds += 1
            # the cumulative table, and what this feed changed: the fed partitions, from their smallest fed day on
            old = {(e, int(d)): int(c) for e, d, c in zip(got_ep.tolist(), got_day.tolist(), got_cnt.tolist())}
            for e, d, c in zip(ep[o].tolist(), day[o].tolist(), share[o].tolist()):
                old[(e, int(d))] = old.get((e, int(d)), 0) + int(c)
            keys = sorted(old)
            got_ep, got_day = np.array([k[0] for k in keys]), np.array([k[1] for k in keys], np.int64)
            got_cnt = np.array([old[k] for k in keys], np.uint64)
            first = {}
            for e, d, c in zip(ep[o].tolist(), day[o].tolist(), share[o].tolist()):
                if c:
                    first[e] = min(first.get(e, d), d)
            want = drop_oracle(got_ep, di, got_day, got_cnt, lambda e, d: e in first and d >= first[e])
            assert rows_map(rows) == want, (d0, part, len(rows), len(want))
            if part == 1:                                      # the endpoints held back arrive in a feed of their own, later
                o = rng.permutation(np.flatnonzero(held_back))
                late_rows = job.feed(ep[o], di[o], day[o], share[o], detection_id="d", partial=True)
                for e, d, c in zip(ep[o].tolist(), day[o].tolist(), share[o].tolist()):
                    old[(e, int(d))] = old.get((e, int(d)), 0) + int(c)
                keys = sorted(old)
                got_ep, got_day = np.array([k[0] for k in keys]), np.array([k[1] for k in keys], np.int64)
                got_cnt = np.array([old[k] for k in keys], np.uint64)
                first = {}
                for e, d in zip(ep[o].tolist(), day[o].tolist()):
                    first[e] = min(first.get(e, d), d)
                assert rows_map(late_rows) == drop_oracle(got_ep, di, got_day, got_cnt, lambda e, d: e in first and d >= first[e]), (d0, "held back")
    assert feeds == 15
    # everything has arrived: the window is the batch job over the whole table
    order = np.lexsort((day, ep))
    assert np.array_equal(got_cnt, cnt[order]) and np.array_equal(got_day, day[order]) and np.array_equal(got_ep, ep[order])
    whole = drop_detection_table(ep, di, day, cnt, detection_id="d", engine=engine)
    assert rows_map(job.window(detection_id="d")) == rows_map(whole) == drop_oracle(ep, di, day, cnt, lambda e, d: True)
    assert len(whole) >= 5
    # the same feed of zeros changes nothing and reports nothing; the default feed still refuses a split day
    assert job.feed(ep[:3], di[:3], day[:3], np.zeros(3, np.uint64), detection_id="d", partial=True) == []
    snap = job.state.export_series()
    with pytest.raises(TadError):
        job.feed(ep[:3], di[:3], day[:3], cnt[:3], detection_id="d")
    assert np.array_equal(job.state.export_series()[1], snap[1])


def oracle_of_counts(want):
    """the drop oracle over a counts table (the pandas query's frame) -> rows in test_gpu_drop_select.keyed's form"""
    import pandas as pd
    if len(want) == 0:
        return []
    codes, uniq = pd.MultiIndex.from_arrays([want["endpoint"], want["direction"]]).factorize()
    day = np.asarray(pd.to_datetime(want["date"]).values.astype("datetime64[D]").astype(np.int64))
    o = dro.run_job(codes.astype(np.uint64), day, want["dropNumber"].to_numpy().astype(np.uint64))
    return sorted((uniq[int(k)][0], uniq[int(k)][1], float(a).hex(), float(s).hex(), str(np.datetime64(int(t), "D")), int(x))
                  for k, t, x, a, s in zip(o["key_id"], o["flow_end_s"], o["throughput"], o["algo_calc"], o["stddev"]))


def query(fl, rows):
    """the pandas query over the flow rows of mask `rows` -> (the rows' columns, the counts frame)"""
    part = {k: v[rows] for k, v in fl["cols"].items()}
    return part, dq.query_pandas(dq.strings_of(part, fl["dict"]), part["ingress_action"], part["egress_action"], part["flow_start_s"], part["flow_end_s"])


def test_the_drop_job_takes_flow_rows_of_a_day_in_three_partial_feeds(engine, flows):  # noqa: F811
    """feed_flows(..., partial=True): drop_select's device columns, key ids from the instance's device dictionary (the state is resized
    as partitions appear), times in seconds of the day's midnight.  Five days at a time, each flow row of the block drawn into one of
    three feeds, so every day of every partition arrives in pieces"""
    from theia_amd import drop_detection as dd
    c, d = flows["cols"], flows["dict"]
    rng = np.random.default_rng(77)
    n = c["flow_start_s"].size
    feed_of = rng.integers(0, 3, n)
    day_of = (c["flow_start_s"] - DAY0) // dq.DAY
    job = dd.PeriodicalDropDetection(engine)
    fed = np.zeros(n, bool)
    reported = again = 0
    for block in range(0, N_DAYS, 5):
        for part in range(3):
            rows = (day_of >= block) & (day_of < block + 5) & (feed_of == part)
            cols, mine = query(flows, rows)
            before = job.state.num_keys if job.state is not None else 0
            got = job.feed_flows(cols, d, detection_id="p", partial=True)
            fed |= rows
            # what this feed changed: its partitions, from their smallest fed day on; judged over everything fed so far
            first = {}
            for e, di, date in zip(mine["endpoint"], mine["direction"], mine["date"]):
                first[(e, di)] = min(first.get((e, di), str(date)), str(date))
            assert first, (block, part)
            want = [r for r in oracle_of_counts(query(flows, fed)[1]) if (r[0], r[1]) in first and r[4] >= first[(r[0], r[1])]]
            assert keyed(got) == want, (block, part, len(got), len(want))
            assert all(r[0] == "periodical" and r[1] == "p" for r in got)
            reported += len(got)
            again += sum(1 for r in want if part > 0 and r[5] == 60)       # a planted day judged again as its count grows
            assert job.state.num_keys >= before
    assert fed.sum() == int(((day_of >= 0) & (day_of < N_DAYS)).sum()) and reported > 0 and again > 0
    # everything has arrived: the window is the batch job over the whole table, planted days and all
    whole = dd.drop_detection_from_flows(engine, c, d, detection_id="p")
    assert keyed(job.window(detection_id="p")) == keyed(whole) == oracle_of_counts(counts_of(flows)[1])
    assert {(r[3], r[4]): str(r[7]) for r in whole if int(r[8]) == 60} == flows["planted"]
    # the same rows again ADD (a merge, not a replace): the feed is judged, the counts double
    series = job.state.export_series()[1].copy()
    last = (day_of == N_DAYS - 1) & (feed_of == 0)
    job.feed_flows(query(flows, last)[0], d, detection_id="p", partial=True)
    assert job.state.export_series()[1].sum() == series.sum() + query(flows, last)[1]["dropNumber"].sum()
    # the default feed still refuses the split day, and changes nothing
    series = job.state.export_series()[1].copy()
    with pytest.raises(TadError):
        job.feed_flows(query(flows, last)[0], d, detection_id="p")
    assert np.array_equal(job.state.export_series()[1], series)
