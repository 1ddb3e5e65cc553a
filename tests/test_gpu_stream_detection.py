"""GPU, end to end: a job with name filters answered from a streaming state (theia_amd/stream_detection.py) equals the batch job over all
rows fed so far.  A seeded flow table — about 3000 rows, 30 pods in 4 namespaces, 6 service port names, 5 external IPs, 60 time steps — is
fed in five shuffled batches to one StreamingAnomalyDetection per mode; every filter the mode has, with and without end_time, for EWMA,
DBSCAN and ARIMA, is compared with anomaly_detection() over the concatenated table with the same arguments: rows sorted by the decoded key
columns and time, every field equal, floats by their bits; the sentinel row without flowStartSeconds.  One drop case:
PeriodicalDropDetection.window(direction=..., namespace=...) equals window() filtered on the host."""
import time

import numpy as np
import pytest

from theia_amd import anomaly_detection as ad
from theia_amd import drop_detection as dd
from theia_amd.stream_detection import StreamingAnomalyDetection
from stream_helpers import IGNORE, IPS, N_STEPS, STEP, SVCS, T0, batches, comparable, keyed, pods

pytestmark = pytest.mark.gpu

ALGOS = ("EWMA", "DBSCAN", "ARIMA")
END = time.strftime(ad.TIME_FORMAT, time.gmtime(T0 + 45 * STEP))


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(3000)
    P = pods()
    assert len({(p[0], p[1]) for p in P}) == 30 and len({p[1] for p in P}) < 30          # a pod name that two namespaces share
    n = 3000
    src, dst = rng.integers(0, 30, n), rng.integers(0, 30, n)
    ext = rng.random(n) < 0.25                              # a quarter of the rows leave the cluster: no destination pod
    no_src = rng.random(n) < 0.05                           # some come from outside: no source pod
    step = rng.integers(0, N_STEPS, n)
    base = 1_000_000_000 * (1 + src % 7) + 300_000_000 * (dst % 5)        # (DBSCAN's default eps is 2.5e8: the spikes must lie further out)
    value = (base + rng.integers(0, 200_000_000, n)) * np.where(rng.random(n) < 0.04, 9, 1)
    col = lambda idx, f, blank: np.where(blank, "", np.array([P[i][f] for i in idx]))
    flows = {
        "sourcePodNamespace": col(src, 0, no_src), "sourcePodName": col(src, 1, no_src), "sourcePodLabels": col(src, 2, no_src),
        "destinationPodNamespace": col(dst, 0, ext), "destinationPodName": col(dst, 1, ext), "destinationPodLabels": col(dst, 2, ext),
        "destinationIP": np.where(ext, np.array(IPS)[rng.integers(0, 5, n)], np.array(["10.0.0.%d" % i for i in dst])),
        "destinationServicePortName": np.where(ext, "", np.array(SVCS)[rng.integers(0, 7, n)]),
        "flowType": np.where(ext, 3, np.where(rng.random(n) < 0.5, 1, 2)).astype(np.int64),
        "flowEndSeconds": (T0 + STEP * step).astype(np.int64), "flowStartSeconds": (T0 + STEP * step - 30).astype(np.int64),
        "throughput": value.astype(np.uint64),
    }
    return flows


# mode, pod_ident -> the filters of the mode as keyword arguments of both calls
FILTERS = {
    ("pod", "name"): [dict(pod_name="web-0"), dict(pod_name="web-0", pod_namespace="shop"), dict(pod_name="db-0", pod_namespace="shop"),
                      dict(pod_name="no-such-pod")],
    ("pod", "labels"): [dict(pod_label="web"), dict(pod_label='"app":"db"', pod_namespace="blog"), dict(), dict(pod_label="no-such-label")],
    ("external", "labels"): [dict(external_ip=IPS[2]), dict(), dict(external_ip="8.8.8.8")],
    ("svc", "labels"): [dict(svc_port_name="shop/web:http"), dict(), dict(svc_port_name="none/none:x")],
}


@pytest.fixture(scope="module")
def fed(engine, table):
    made = {}
    for mode, ident in FILTERS:
        s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
        for b in batches(table):
            s.feed(b)
        made[(mode, ident)] = s
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("mode,ident", sorted(FILTERS))
def test_job_from_the_state_equals_the_batch_job_over_all_rows(engine, table, fed, mode, ident, algo):
    s = fed[(mode, ident)]
    assert s.num_keys > 3 and s.state.num_keys == s.num_keys
    real, sentinel = 0, 0
    for filt in FILTERS[(mode, ident)]:
        for end_time in ("", END):
            _, want = ad.anomaly_detection(algo, table, "", end_time, "job-1", IGNORE, mode, engine=engine, **filt)
            _, got = s.job(algo, "job-1", end_time=end_time, **filt)
            print(mode, ident, algo, filt, repr(end_time), "rows:", len(want), want[0]["anomaly"])
            assert comparable(got, s.mode) == comparable(want, s.mode), (mode, ident, algo, filt, end_time)
            if want[0]["anomaly"] == "true":
                real += 1
                if mode != "pod" and end_time:
                    assert max(r["flowEndSeconds"] for r in got) < ad._epoch(END)
                names = {"pod_name": "podName", "external_ip": "destinationIP", "svc_port_name": "destinationServicePortName"}
                for arg, colname in names.items():
                    if arg in filt:
                        assert {r[colname] for r in got} == {filt[arg]}
                if "pod_namespace" in filt:
                    assert {r["podNamespace"] for r in got} == {filt["pod_namespace"]}
            else:
                sentinel += 1
                assert len(got) == 1
    assert real >= 2 and sentinel >= 2, (real, sentinel)      # filters that find anomalies, and the one that matches nothing


def test_what_the_feed_and_the_job_refuse(engine, table):
    with pytest.raises(ValueError):
        StreamingAnomalyDetection(engine, "")
    with pytest.raises(ValueError):
        StreamingAnomalyDetection(engine, "pod", pod_ident="uid")
    s = StreamingAnomalyDetection(engine, "pod", pod_ident="labels")
    assert s.job("EWMA", "j")[1][0]["anomaly"] == "NO ANOMALY DETECTED"     # nothing fed yet
    s.feed(next(batches(table)))
    with pytest.raises(ValueError):
        s.job("EWMA", "j", pod_name="web-0")                  # keyed by labels: a job by name needs the other key set
    with pytest.raises(ValueError):
        s.job("KMEANS", "j")
    s.close()
    s = StreamingAnomalyDetection(engine, "pod", pod_ident="name")
    s.feed(next(batches(table)))
    with pytest.raises(ValueError):
        s.job("EWMA", "j", pod_label="web")
    with pytest.raises(ValueError):
        s.job("EWMA", "j")
    s.close()


# ---- the drop job: partitions selected by direction and namespace ----
def drop_flows():
    rng = np.random.default_rng(77)
    d = {"ip": ["10.9.0.%d" % i for i in range(30)], "pod_ns": ["ns-a", "ns-b", "ns-c"], "pod_name": [""] + ["pod-%d" % i for i in range(24)]}
    ep, day = [], []
    for e in range(24):
        counts = rng.integers(5, 10, 14)
        if e % 5 != 4:
            counts[int(rng.integers(0, 14))] = 70          # 14 days: one outlier among them lies 3.3 sample std from the mean
        for dy, k in enumerate(counts):
            ep += [e] * int(k)
            day += [dy] * int(k)
    ep, day = np.array(ep), np.array(day)
    o = rng.permutation(ep.size)
    ep, day = ep[o], day[o]
    n = ep.size
    ingress, pod = (ep // 2) % 2 == 0, ep % 4 != 3          # every fourth endpoint is an IP
    zeros = np.zeros(n, np.int64)
    c = {"ingress_action": np.where(ingress, 2, 0).astype(np.uint8), "egress_action": np.where(ingress, 0, 3).astype(np.uint8),
         "flow_start_s": 1660176000 + day * 86400 + rng.integers(0, 86400, n)}
    for side, mine in (("dst", ingress), ("src", ~ingress)):
        c[side + "_ip"] = np.where(mine, ep, 29).astype(np.int64)
        c[side + "_pod_ns"] = np.where(mine & pod, ep % 3, zeros).astype(np.int64)
        c[side + "_pod_name"] = np.where(mine & pod, 1 + ep, zeros).astype(np.int64)
    return c, d


def test_drop_window_by_direction_and_namespace(engine):
    c, d = drop_flows()
    p = dd.PeriodicalDropDetection(engine)
    for lo, hi in ((0, 7), (7, 14)):                         # two feeds of whole days
        rows = (c["flow_start_s"] >= 1660176000 + lo * 86400) & (c["flow_start_s"] < 1660176000 + hi * 86400)
        p.feed_flows({k: v[rows] for k, v in c.items()}, d, detection_id="p")
    everything = p.window(detection_id="w")
    assert len(everything) >= 10 and {r[4] for r in everything} == {"ingress", "egress"}
    assert any(not r[3].startswith("ns-") for r in everything) and {r[3][:4] for r in everything if "/" in r[3]} == {"ns-a", "ns-b", "ns-c"}
    cases = {("ingress", None): lambda r: r[4] == "ingress", ("egress", None): lambda r: r[4] == "egress",
             (None, "ns-b"): lambda r: r[3].startswith("ns-b/"), ("ingress", "ns-a"): lambda r: r[4] == "ingress" and r[3].startswith("ns-a/"),
             ("egress", "ns-zz"): lambda r: False}
    for (direction, namespace), rule in cases.items():
        got = p.window(detection_id="w", direction=direction, namespace=namespace)
        want = [r for r in everything if rule(r)]
        assert keyed(got) == keyed(want), (direction, namespace)
        assert len(want) > 0 or namespace == "ns-zz"
    got = p.window("2022-08-13", "2022-08-24", detection_id="w", direction="ingress")        # with a range of days on top
    assert keyed(got) == keyed([r for r in p.window("2022-08-13", "2022-08-24", detection_id="w") if r[4] == "ingress"])
    with pytest.raises(ValueError):
        p.window(direction="sideways")
    by_counts = dd.PeriodicalDropDetection(engine)            # an instance fed counts has no device dictionary to select on
    by_counts.feed(["a", "a", "a"], ["ingress"] * 3, ["2022-08-11", "2022-08-12", "2022-08-13"], [1, 2, 3])
    with pytest.raises(ValueError):
        by_counts.window(direction="ingress")
    assert by_counts.window() == []
