"""GPU, end to end: a --pod-label with LIKE wildcards answered from a streaming state, on the device.  The table of
tests/test_gpu_stream_detection.py with label sets whose keys hold '_' — the reference's documented example is
--pod-label "test_key":"test_value", and _ is a wildcard in the ilike the job builds.  Every job returns the rows of anomaly_detection()
over everything fed, with the same arguments; around job() the batch job's regex (_like_regex) is called 0 times and StringDict.like at
least once.  A non-ASCII pattern still takes the host regex and still agrees."""
import struct

import numpy as np
import pytest

from theia_amd import StringDict
from theia_amd import anomaly_detection as ad
from theia_amd.stream_detection import StreamingAnomalyDetection

pytestmark = pytest.mark.gpu

T0 = 1660202800
STEP = 60
N_STEPS = 60
NAMESPACES = ("shop", "blog", "infra", "kube-system")
IGNORE = ("kube-system",)
LABELS = ('{"app":"web","test_key":"test_value"}', '{"app":"db","testXkey":"test-value"}', '{"app":"cache","zone":"db","TEST_KEY":"TEST_VALUE"}',
          '{"app":"Web-Front","tier":"100%"}', '{"app":"café","test_key":"other"}')


def pods():
    """30 pods: (namespace, labels); every label set is its own, and carries a key the result drops"""
    return [(NAMESPACES[i % 4], LABELS[i % 5][:-1] + ',"idx":"p%d","pod-template-hash":"h%d"}' % (i, i)) for i in range(30)]


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(3100)
    P = pods()
    n = 2400
    src, dst = rng.integers(0, 30, n), rng.integers(0, 30, n)
    ext = rng.random(n) < 0.2
    step = rng.integers(0, N_STEPS, n)
    base = 1_000_000_000 * (1 + src % 7) + 300_000_000 * (dst % 5)        # (DBSCAN's default eps is 2.5e8: the spikes must lie further out)
    value = (base + rng.integers(0, 200_000_000, n)) * np.where(rng.random(n) < 0.04, 9, 1)
    col = lambda idx, f, blank: np.where(blank, "", np.array([P[i][f] for i in idx]))
    never = np.zeros(n, dtype=bool)
    return {
        "sourcePodNamespace": col(src, 0, never), "sourcePodName": np.array(["p%d" % i for i in src]), "sourcePodLabels": col(src, 1, never),
        "destinationPodNamespace": col(dst, 0, ext), "destinationPodName": np.where(ext, "", np.array(["p%d" % i for i in dst])), "destinationPodLabels": col(dst, 1, ext),
        "destinationIP": np.array(["10.0.0.%d" % i for i in dst]), "destinationServicePortName": np.where(ext, "", "shop/web:http"),
        "flowType": np.where(ext, 3, 1).astype(np.int64),
        "flowEndSeconds": (T0 + STEP * step).astype(np.int64), "flowStartSeconds": (T0 + STEP * step - 30).astype(np.int64),
        "throughput": value.astype(np.uint64),
    }


@pytest.fixture(scope="module")
def fed(engine, table):
    s = StreamingAnomalyDetection(engine, "pod", pod_ident="labels", ns_ignore_list=IGNORE)
    n = len(table["flowEndSeconds"])
    part = np.random.default_rng(8).integers(0, 4, n)
    for p in (2, 0, 3, 1):
        rows = np.random.default_rng(20 + p).permutation(np.flatnonzero(part == p))
        s.feed({k: v[rows] for k, v in table.items()})
    yield s
    s.close()


def comparable(rows, mode):
    """result rows -> sorted tuples; floats as bit patterns; the sentinel row without its flowStartSeconds (the time it was made)"""
    out = []
    for r in rows:
        r = dict(r)
        if r.get("anomaly") == "NO ANOMALY DETECTED":
            r.pop("flowStartSeconds")
        out.append(tuple((k, struct.pack("<d", v).hex() if isinstance(v, float) else v) for k, v in sorted(r.items())))
    key = lambda t: tuple(str(dict(t).get(c)) for c in ad.KEY_COLUMNS[mode]) + (dict(t)["flowEndSeconds"],)
    return sorted(out, key=key)


def counted_job(monkeypatch, s, algo, **filt):
    """s.job(...) with the two routes counted: -> (rows, calls of _like_regex, calls of StringDict.like)"""
    calls = {"regex": 0, "like": []}
    regex, like = ad._like_regex, StringDict.like

    def counting_regex(pattern):
        calls["regex"] += 1
        return regex(pattern)

    def counting_like(self, pattern, nocase=False, out="host"):
        calls["like"].append((pattern, nocase, out))
        return like(self, pattern, nocase=nocase, out=out)

    with monkeypatch.context() as m:
        m.setattr(ad, "_like_regex", counting_regex)
        m.setattr(StringDict, "like", counting_like)
        _, got = s.job(algo, "job-1", **filt)
    return got, calls["regex"], calls["like"]


# the filter, and whether it selects some pods (a job with anomalies) or none (the sentinel row)
DEVICE_JOBS = [
    (dict(pod_label='"test_key":"test_value"'), True),                  # the reference's documented example: _ matches X and -, the fold TEST_KEY
    (dict(pod_label="app%db"), True),                                   # "app":"db" and "app":"cache","zone":"db"
    (dict(pod_label="test\\_key"), True),                               # the escaped _: test_key and TEST_KEY, not testXkey
    (dict(pod_label='"test_key":"test_value"', pod_namespace="blog"), True),
    (dict(pod_label="100\\%"), True),                                   # a literal %
    (dict(pod_label="test_key_:_no-such-value"), False),
]


@pytest.mark.parametrize("algo", ("EWMA", "DBSCAN"))
def test_a_wildcard_label_is_answered_on_the_device_and_equals_the_batch_job(engine, table, fed, monkeypatch, algo):
    real = 0
    for filt, finds in DEVICE_JOBS:
        _, want = ad.anomaly_detection(algo, table, "", "", "job-1", IGNORE, "pod", engine=engine, **filt)
        got, n_regex, likes = counted_job(monkeypatch, fed, algo, **filt)
        print(algo, filt, "rows:", len(want), want[0]["anomaly"])
        assert comparable(got, fed.mode) == comparable(want, fed.mode), (algo, filt)
        assert n_regex == 0 and likes == [("%" + filt["pod_label"] + "%", True, "device")], (filt, n_regex, likes)
        assert (want[0]["anomaly"] == "true") == finds, filt
        if finds:
            real += 1
            if "pod_namespace" in filt:
                assert {r["podNamespace"] for r in got} == {"blog"}
    assert real >= 4


def test_the_selections_differ_as_the_wildcards_say(engine, fed):
    """the three label patterns select three different key sets: the jobs above did not agree by selecting everything or nothing"""
    vocab = fed._vocab[1]
    labels = vocab.values().to_pylist()
    masks = {}
    for label in ('"test_key":"test_value"', "test\\_key", "app%db", "100\\%"):
        mask, hit = vocab.like("%" + label + "%", nocase=True)
        rx = ad._like_regex("%" + label + "%")
        assert mask.tolist() == [1 if rx.match(s) else 0 for s in labels], label
        assert 0 < hit < len(labels), label
        masks[label] = mask.tobytes()
    assert len(set(masks.values())) == len(masks)


def test_a_wildcard_free_label_and_a_non_ascii_one_keep_their_routes(engine, table, fed, monkeypatch):
    # (filter, calls of the regex, calls of StringDict.like, finds pods).  _ is ONE character: é is one, its two bytes are not two
    cases = ((dict(pod_label="web"), 0, 0, True), (dict(pod_label="CAFÉ"), 1, 0, True), (dict(pod_label='caf_",'), 0, 1, True), (dict(pod_label='caf__",'), 0, 1, False),
             (dict(pod_label="café_,"), 1, 0, True))
    for filt, n_regex_want, n_like_want, finds in cases:
        _, want = ad.anomaly_detection("EWMA", table, "", "", "job-1", IGNORE, "pod", engine=engine, **filt)
        got, n_regex, likes = counted_job(monkeypatch, fed, "EWMA", **filt)
        assert comparable(got, fed.mode) == comparable(want, fed.mode), filt
        assert (n_regex, len(likes)) == (n_regex_want, n_like_want), filt
        assert (want[0]["anomaly"] == "true") == finds, filt
