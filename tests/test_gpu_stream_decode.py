"""GPU, end to end: a StreamingAnomalyDetection that keeps no key table on the host.  A seeded flow table — 6000 rows, a few hundred keys
per mode, 40 time steps — is fed in five shuffled batches; job() must equal anomaly_detection() over all rows, the result rows' strings
coming from KeyDict.gather and StringDict.decode alone.  Restart: after three feeds snapshot() -> restore() into a second instance, the
last two batches go to both, and both must give the batch job's rows — among them the rows of a key whose strings occur only in the
batches before the snapshot."""
import struct

import numpy as np
import pytest

from theia_amd import anomaly_detection as ad
from theia_amd import stream_detection as sd
from theia_amd.stream_detection import StreamingAnomalyDetection

pytestmark = pytest.mark.gpu

T0 = 1660202800
STEP = 60
N_STEPS = 40
N_ROWS = 6000
PARTS = 5
NAMESPACES = ("shop", "blog", "infra", "kube-system")
IGNORE = ("kube-system",)
EARLY = {"svc": "early/only:http", "ip": "52.9.9.9", "pod": "early-0", "labels": '{"app":"early","pod-template-hash":"e0"}'}
MODES = [("svc", "labels"), ("external", "labels"), ("pod", "labels"), ("pod", "name")]
# per mode: the job that shows the early key (no filter; an instance keyed by pod names serves jobs with pod_name only), and one name filter
FILTERS = {("svc", "labels"): [dict(), dict(svc_port_name="ns7/svc7:http")], ("external", "labels"): [dict(), dict(external_ip="52.1.0.7")],
           ("pod", "labels"): [dict(), dict(pod_label='"app":"app2"')],
           ("pod", "name"): [dict(pod_name=EARLY["pod"]), dict(pod_name="app2-1", pod_namespace="infra")]}
EARLY_COLUMN = {("svc", "labels"): ("destinationServicePortName", EARLY["svc"]), ("external", "labels"): ("destinationIP", EARLY["ip"]),
                ("pod", "labels"): ("podLabels", '{"app": "early"}'), ("pod", "name"): ("podName", EARLY["pod"])}


def build_table():
    rng = np.random.default_rng(4100)
    pods = [(NAMESPACES[i % 4], "app%d-%d" % (i % 12, i // 12), '{"app":"app%d","pod-template-hash":"h%d","tier":"t%d"}' % (i % 12, i, i // 12)) for i in range(150)]
    pods.append(("shop", EARLY["pod"], EARLY["labels"]))
    svcs = np.array([""] + ["ns%d/svc%d:http" % (i % 9, i) for i in range(200)] + [EARLY["svc"]])
    ips = np.array(["52.1.0.%d" % i for i in range(200)] + [EARLY["ip"]])
    n = N_ROWS
    src, dst = rng.integers(0, 150, n), rng.integers(0, 150, n)
    ext = rng.random(n) < 0.3
    step = rng.integers(0, N_STEPS, n)
    svc = rng.integers(0, 201, n)
    ip = rng.integers(0, 200, n)
    early = np.zeros(n, dtype=bool)
    early[:N_STEPS] = True                                   # the first 40 rows: one key per mode that only the early batches see
    src[early], dst[early], svc[early], ip[early], step[early] = 150, 150, 201, 200, np.arange(N_STEPS)
    ext[early] = np.arange(N_STEPS) % 2 == 0                 # half of them leave the cluster (external mode), half reach the service
    base = 1_000_000_000 * (1 + src % 7) + 300_000_000 * (dst % 5)
    value = (base + rng.integers(0, 200_000_000, n)) * np.where(rng.random(n) < 0.04, 9, 1)
    value[early] = 1_000_000_000 + np.arange(N_STEPS) * 1000
    value[[20, 21]] *= 40                                    # the early key's spike, in both halves
    col = lambda idx, f, blank: np.where(blank, "", np.array([pods[i][f] for i in idx]))
    nobody = np.zeros(n, dtype=bool)
    flows = {
        "sourcePodNamespace": col(src, 0, nobody), "sourcePodName": col(src, 1, nobody), "sourcePodLabels": col(src, 2, nobody),
        "destinationPodNamespace": col(dst, 0, ext), "destinationPodName": col(dst, 1, ext), "destinationPodLabels": col(dst, 2, ext),
        "destinationIP": np.where(ext, ips[ip], np.array(["10.0.0.%d" % (i % 250) for i in dst])),
        "destinationServicePortName": np.where(ext, "", svcs[svc]),
        "flowType": np.where(ext, 3, 1).astype(np.int64),
        "flowEndSeconds": (T0 + STEP * step).astype(np.int64), "flowStartSeconds": (T0 + STEP * step - 30).astype(np.int64),
        "throughput": value.astype(np.uint64),
    }
    part = rng.integers(0, PARTS, n)
    part[early] = np.arange(N_STEPS) % 3                      # ... parts 0, 1 and 2 only
    batches = []
    for p in range(PARTS):
        rows = np.random.default_rng(50 + p).permutation(np.flatnonzero(part == p))
        batches.append({k: v[rows] for k, v in flows.items()})
    return flows, batches


@pytest.fixture(scope="module")
def table():
    return build_table()


def comparable(rows, mode):
    out = []
    for r in rows:
        r = dict(r)
        if r.get("anomaly") == "NO ANOMALY DETECTED":
            r.pop("flowStartSeconds")
        out.append(tuple((k, struct.pack("<d", v).hex() if isinstance(v, float) else v) for k, v in sorted(r.items())))
    key = lambda t: tuple(str(dict(t).get(c)) for c in ad.KEY_COLUMNS[mode]) + (dict(t)["flowEndSeconds"],)
    return sorted(out, key=lambda t: (key(t), t))


@pytest.fixture(scope="module")
def fed(engine, table):
    """per mode: (the instance fed all five batches, the instance restored after three and fed the last two)"""
    _, batches = table
    made = {}
    for mode, ident in MODES:
        s = StreamingAnomalyDetection(engine, mode, pod_ident=ident, ns_ignore_list=IGNORE)
        for b in batches[:3]:
            s.feed(b)
        snap = s.snapshot()
        assert all(isinstance(v, np.ndarray) for v in snap.values())
        r = StreamingAnomalyDetection.restore(engine, snap, mode, pod_ident=ident, ns_ignore_list=IGNORE)
        for b in batches[3:]:
            s.feed(b)
            r.feed(b)
        made[(mode, ident)] = (s, r)
    yield made
    for s, r in made.values():
        s.close()
        r.close()


@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN"])
@pytest.mark.parametrize("mode,ident", MODES)
def test_job_equals_the_batch_job_before_and_after_a_restart(engine, table, fed, mode, ident, algo):
    flows, _ = table
    s, r = fed[(mode, ident)]
    real = 0
    for i, filt in enumerate(FILTERS[(mode, ident)]):
        _, want = ad.anomaly_detection(algo, flows, "", "", "job-1", IGNORE, mode, engine=engine, **filt)
        _, got = s.job(algo, "job-1", **filt)
        _, again = r.job(algo, "job-1", **filt)
        print(mode, ident, algo, filt, "rows:", len(want), want[0]["anomaly"])
        assert comparable(got, s.mode) == comparable(want, s.mode), (mode, ident, algo, filt)
        assert comparable(again, s.mode) == comparable(want, s.mode), (mode, ident, algo, filt, "restored")
        real += want[0]["anomaly"] == "true"
        if i == 0 and algo == "EWMA":
            # the key that only the batches before the snapshot named: its strings come out of the restored dictionaries
            name, value = EARLY_COLUMN[(mode, ident)]
            assert any(row[name] == value for row in want), "the early key has no anomalous point: the case shows nothing"
            assert any(row[name] == value for row in again)
    assert real >= 1


@pytest.mark.parametrize("mode,ident", MODES)
def test_nothing_on_the_host_grows_with_the_keys(fed, mode, ident):
    s, r = fed[(mode, ident)]
    for inst in (s, r):
        assert not hasattr(inst, "_keys")
        assert inst.num_keys == inst._dict.num_keys() == inst.state.num_keys and inst.num_keys > 100
        for name, v in vars(inst).items():
            assert not isinstance(v, (dict, set, np.ndarray)), name
            if isinstance(v, (list, tuple)):
                assert len(v) <= 2, name                      # the string dictionaries, the ignore list
    assert s.num_keys == r.num_keys


@pytest.mark.parametrize("mode,ident", MODES)
def test_every_key_decodes_alike_in_the_restored_instance(fed, mode, ident):
    s, r = fed[(mode, ident)]
    ids = np.arange(s.num_keys, dtype=np.uint64)
    a = sd._KeyDecoder(s._dict, s._vocab).columns(ids)
    b = sd._KeyDecoder(r._dict, r._vocab).columns(ids)
    assert len(a) == len(b) == len(s._vocab) + 1
    for x, y in zip(a, b):
        assert x.tolist() == y.tolist()
    wanted = {"svc": EARLY["svc"], "external": EARLY["ip"]}.get(mode) or (EARLY["labels"] if ident == "labels" else EARLY["pod"])
    assert wanted in b[-2].tolist()
