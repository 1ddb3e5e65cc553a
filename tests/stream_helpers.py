"""What the StreamDetection-level tests share: the cluster of the flow tables (pods, services, addresses), the tables as batches, the
fake table client that serves rows by arrival, result rows in a comparable form, what an instance's state holds, and the fixtures `table`
(two of them: one per family, each registered under that name in the module that imports it) and `flows`."""
import re
import struct

import numpy as np
import pytest

import drop_query_ref as dq
from theia_amd import anomaly_detection as ad
from theia_amd.stream_detection import _KeyColumn, _KeyDecoder

T0 = 1660202800
STEP = 60
N_STEPS = 60
NAMESPACES = ("shop", "blog", "infra", "kube-system")
IGNORE = ("kube-system",)
SVCS = ["", "shop/web:http", "shop/db:pg", "blog/web:http", "infra/dns:udp", "infra/log:tcp", "blog/cache:mc"]
IPS = ["52.1.0.%d" % i for i in range(5)]


def pods():
    """30 pods: (namespace, name, labels).  web-0 exists in two namespaces; labels carry keys the result drops"""
    out = []
    for i in range(30):
        ns = NAMESPACES[i % 4]
        app = ("web", "db", "cache", "Web-Front", "dns")[i % 5]
        name = "%s-%d" % (app.lower(), i // 20)
        labels = '{"app":"%s","pod-template-hash":"h%d","tier":"t%d"}' % (app, i, i % 3)
        out.append((ns, name, labels))
    return out


def batches(flows, parts=5, seed=7):
    n = len(flows["flowEndSeconds"])
    part = np.random.default_rng(seed).integers(0, parts, n)
    for p in np.random.default_rng(seed + 1).permutation(parts):
        rows = np.random.default_rng(seed + 2 + p).permutation(np.flatnonzero(part == p))
        yield {k: v[rows] for k, v in flows.items()}


def f64_bits(x):
    return struct.pack("<d", float(x)).hex()


def comparable(rows, mode):
    """result rows -> sorted tuples; floats as bit patterns; the sentinel row without its flowStartSeconds (the time it was made)"""
    out = []
    for r in rows:
        r = dict(r)
        if r.get("anomaly") == "NO ANOMALY DETECTED":
            r.pop("flowStartSeconds")
        out.append(tuple((k, f64_bits(v) if isinstance(v, float) else v) for k, v in sorted(r.items())))
    key = lambda t: tuple(str(dict(t).get(c)) for c in ad.KEY_COLUMNS[mode]) + (dict(t)["flowEndSeconds"],)
    return sorted(out, key=key)


LAG = 4 * STEP
MODES = [("svc", "labels"), ("pod", "labels"), ("pod", "name")]


@pytest.fixture(name="table", scope="module")
def replace_table():
    """test_gpu_stream_detection's table at 5000 rows, and each row's arrival time: up to three steps after its flowEndSeconds"""
    rng = np.random.default_rng(5000)
    P = pods()
    n = 5000
    src, dst = rng.integers(0, 30, n), rng.integers(0, 30, n)
    ext = rng.random(n) < 0.25
    no_src = rng.random(n) < 0.05
    step = rng.integers(0, N_STEPS, n)
    base = 1_000_000_000 * (1 + src % 7) + 300_000_000 * (dst % 5)
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
    arrival = flows["flowEndSeconds"] + rng.integers(0, 3 * STEP + 1, n)
    return flows, arrival


class TableClient:
    """what poll needs of a ClickHouseHTTP: query_columns(sql) answered from the table — the rows that have arrived by `self.now` inside
    the range the SQL names (the row predicates are left to the feed, which applies them again)"""

    def __init__(self, flows, arrival):
        self.flows, self.arrival, self.now, self.queries = flows, arrival, 0, []

    def query_columns(self, sql, dict_strings=False, **kw):
        self.queries.append(sql)
        lo = re.search(r"flowEndSeconds >= toDateTime\((\d+)\)", sql)
        hi = re.search(r"flowEndSeconds < toDateTime\((\d+)\)", sql)
        t = self.flows["flowEndSeconds"]
        sel = (self.arrival <= self.now) & (t < int(hi.group(1)))
        if lo:
            sel &= t >= int(lo.group(1))
        rows = np.random.default_rng(len(self.queries)).permutation(np.flatnonzero(sel))
        names = sql[len("SELECT "):sql.index(" FROM ")].split(", ")
        return {c: self.flows[c][rows] for c in names} if rows.size else {}


def turns():
    """the `now` of the eight polls: every 8 steps, the last one late enough for every row to have arrived"""
    return [T0 + STEP * 8 * (p + 1) + (3 * STEP + 1 if p == 7 else 0) for p in range(8)]


def key_tuples(s):
    """key id -> the key's tuple in the mode's result columns"""
    decoder = _KeyDecoder(s._dict, s._vocab)
    cols = [np.asarray(_KeyColumn(decoder, "direction" if name == "direction" else i)) for i, name in enumerate(ad.KEY_COLUMNS[s.mode])]
    for i, name in enumerate(ad.KEY_COLUMNS[s.mode]):
        if name == "podLabels":      # (the result rows carry the canonical labels; the table's pods stay distinct under it)
            cols[i] = np.asarray([ad.remove_meaningless_labels(v) for v in cols[i]], dtype=object)
    tuples = [tuple(str(c[k]) for c in cols) for k in range(s.num_keys)]
    assert len(set(tuples)) == len(tuples), ("key_tuples", "two key ids decode to one tuple")
    return tuples


def held(s):
    """-> {key id: {time: value}} of everything the instance's state holds"""
    if s.state is None:
        return {}
    ln, vals = s.state.export_series()
    times = s.state.export_times() if vals.size else np.zeros(0, np.int64)
    out, at = {}, 0
    for k, n in enumerate(ln.astype(np.int64).tolist()):
        out[k] = dict(zip(times[at:at + n].tolist(), vals[at:at + n].tolist()))
        at += n
    return out


def changed_since(before, after):
    """{key id: the smallest time at which the key's points differ}"""
    out = {}
    for k, pts in after.items():
        old = before.get(k, {})
        ts = [t for t in set(pts) | set(old) if pts.get(t) != old.get(t)]
        if ts:
            out[k] = min(ts)
    return out


SPAN = 3600                  # an hour of seconds from T0 (which is not on a minute)
BUCKET = 60


@pytest.fixture(name="table", scope="module")
def seconds_table():
    """test_gpu_stream_detection's table with flowEndSeconds at seconds, not minutes, and each row's arrival up to 150 s later"""
    rng = np.random.default_rng(6000)
    P = pods()
    n = 6000
    src, dst = rng.integers(0, 30, n), rng.integers(0, 30, n)
    ext = rng.random(n) < 0.25
    no_src = rng.random(n) < 0.05
    sec = rng.integers(0, SPAN, n)
    base = 100_000_000 * (1 + src % 7) + 30_000_000 * (dst % 5)
    value = (base + rng.integers(0, 20_000_000, n)) * np.where((sec // 60) % 13 == 5, 9, 1)      # some minutes carry nine times the traffic
    col = lambda idx, f, blank: np.where(blank, "", np.array([P[i][f] for i in idx]))
    flows = {
        "sourcePodNamespace": col(src, 0, no_src), "sourcePodName": col(src, 1, no_src), "sourcePodLabels": col(src, 2, no_src),
        "destinationPodNamespace": col(dst, 0, ext), "destinationPodName": col(dst, 1, ext), "destinationPodLabels": col(dst, 2, ext),
        "destinationIP": np.where(ext, np.array(IPS)[rng.integers(0, 5, n)], np.array(["10.0.0.%d" % i for i in dst])),
        "destinationServicePortName": np.where(ext, "", np.array(SVCS)[rng.integers(0, 7, n)]),
        "flowType": np.where(ext, 3, np.where(rng.random(n) < 0.5, 1, 2)).astype(np.int64),
        "flowEndSeconds": (T0 + sec).astype(np.int64), "flowStartSeconds": (T0 + sec - 30).astype(np.int64),
        "throughput": value.astype(np.uint64),
    }
    assert T0 % BUCKET != 0 and np.unique(flows["flowEndSeconds"] % BUCKET).size == BUCKET, ("table", "the seconds do not cover a bucket")
    arrival = flows["flowEndSeconds"] + rng.integers(0, 151, n)
    return flows, arrival


DAY0 = 1660176000       # a midnight
N_ENDPOINTS, N_DAYS, PLANTED, SHORT = 40, 20, (3, 11, 18, 26, 37), (5, 20, 33)
DROP_PAIRS = np.array([(2, 0), (3, 1), (0, 2), (4, 3), (2, 3), (3, 2), (255, 2), (2, 255), (3, 3)], dtype=np.uint8)
PASS_PAIRS = np.array([(a, b) for a in (0, 1, 4, 255) for b in (0, 1, 4, 255)], dtype=np.uint8)


def flow_table(n, selected, seed=0):
    """n flow rows whose ACTIONS select exactly the rows of `selected`; pod-name code 0 means "no pod" on about a third of the sides"""
    rng = np.random.default_rng(1000 + seed)
    selected = np.asarray(selected, dtype=bool)
    pairs = np.where(selected[:, None], DROP_PAIRS[rng.integers(0, len(DROP_PAIRS), n)], PASS_PAIRS[rng.integers(0, len(PASS_PAIRS), n)])
    c = {"ingress_action": np.ascontiguousarray(pairs[:, 0]), "egress_action": np.ascontiguousarray(pairs[:, 1])}
    for side in ("src", "dst"):
        c[side + "_ip"] = rng.integers(0, 50, n)
        c[side + "_pod_ns"] = rng.integers(0, 5, n)
        c[side + "_pod_name"] = np.where(rng.random(n) < 0.33, 0, rng.integers(1, 20, n))
    c["flow_start_s"] = DAY0 + rng.integers(0, 20 * dq.DAY, n)
    c["flow_end_s"] = c["flow_start_s"] + rng.integers(0, 3600, n)
    return c


@pytest.fixture(scope="module")
def flows():
    rng = np.random.default_rng(20260)
    dictionaries = {"ip": ["10.1.%d.%d" % (i // 8, i % 8) for i in range(N_ENDPOINTS + 10)], "pod_ns": ["ns-a", "ns-b", "ns-c", "ns-d", "ns-e"],
                    "pod_name": [""] + ["pod-%d" % i for i in range(N_ENDPOINTS)]}
    ep, day = [], []
    planted = {}
    for e in range(N_ENDPOINTS):
        days = [4, 13] if e in SHORT else list(range(N_DAYS))
        counts = rng.integers(5, 10, len(days))
        if e in PLANTED:
            j = int(rng.integers(0, N_DAYS))
            counts[j] = 60
            planted[e] = j
        for d, k in zip(days, counts):
            ep += [e] * int(k)
            day += [d] * int(k)
    ep, day = np.array(ep), np.array(day)
    m = ep.size
    n = 31 * m                                   # unselected rows mixed in at 30 : 1
    at = np.sort(rng.choice(n, m, replace=False))
    order = rng.permutation(m)
    ep, day = ep[order], day[order]
    c = flow_table(n, np.zeros(n, bool), seed=99)
    pod, ingress = ep % 2 == 0, (ep // 2) % 2 == 0
    also = rng.random(m) < 0.2                   # some rows drop on both sides: ingress wins
    c["ingress_action"][at] = np.where(ingress, rng.choice([2, 3], m), rng.choice([0, 1, 4], m)).astype(np.uint8)
    c["egress_action"][at] = np.where(ingress, np.where(also, 3, 0), rng.choice([2, 3], m)).astype(np.uint8)
    for side, mine in (("dst", ingress), ("src", ~ingress)):
        c[side + "_ip"][at] = np.where(mine, ep, c[side + "_ip"][at])
        c[side + "_pod_ns"][at] = np.where(mine, ep % 3, c[side + "_pod_ns"][at])
        c[side + "_pod_name"][at] = np.where(mine, np.where(pod, 1 + ep, 0), c[side + "_pod_name"][at])
    c["flow_start_s"] = DAY0 + rng.integers(0, N_DAYS, n) * dq.DAY + rng.integers(0, dq.DAY, n)
    c["flow_start_s"][at] = DAY0 + day * dq.DAY + rng.integers(0, dq.DAY, m)
    c["flow_end_s"] = c["flow_start_s"] + 60
    name = lambda e: ("ns-%s/pod-%d" % ("abc"[e % 3], e) if e % 2 == 0 else dictionaries["ip"][e], "ingress" if (e // 2) % 2 == 0 else "egress")
    return {"cols": c, "dict": dictionaries, "planted": {name(e): str(np.datetime64(DAY0 + j * dq.DAY, "s").astype("datetime64[D]")) for e, j in planted.items()},
            "short": [name(e) for e in SHORT], "m": m}


def keyed(rows):
    """result tuples -> comparable rows: endpoint, direction, mean and std as bit patterns, date, number"""
    return sorted((r[3], r[4], float(r[5]).hex(), float(r[6]).hex(), str(r[7]), int(r[8])) for r in rows)


def counts_of(flows, lo=0, hi=N_DAYS):
    """the pandas query over the rows whose start lies in days [lo, hi)"""
    c = flows["cols"]
    rows = (c["flow_start_s"] >= DAY0 + lo * dq.DAY) & (c["flow_start_s"] < DAY0 + hi * dq.DAY)
    part = {k: v[rows] for k, v in c.items()}
    return part, dq.query_pandas(dq.strings_of(part, flows["dict"]), part["ingress_action"], part["egress_action"], part["flow_start_s"], part["flow_end_s"])
