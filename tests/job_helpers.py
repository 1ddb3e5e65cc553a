"""What the batch-job and ingest tests share: the job against the oracle (`check_job`), the request cases of the host job and their canonical
form, the tables and checks of the sparse Stage 0, the narrow-column plans, the flow table of the end-to-end tests, strings and key tuples
as columns on the host and on the device, what a dictionary holds (`exported`, `keydict_snapshot`), and the `#define`s of include/tad.h."""
import json
import os
import re

import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import _capi as capi
from theia_amd.engine import DeviceArray

SKIP = np.uint64(capi.TAD_KEY_SKIP)
SKIP64 = np.uint64(orc.MASK64)
SKIP32 = np.uint32(0xFFFFFFFF)
STAGE = 24 * 1024          # kSeStage: a block of 256 rows whose bytes span more than this reads them lane by lane
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "tad.h")).read()


def header_define(name):
    m = re.search(r"#define %s\s+(\S+)" % name, HEADER)
    assert m, ("no #define in include/tad.h", name)
    return m.group(1)


def check_job(engine, algo, key, t, v, num_keys, agg_flow="svc", **kw):
    okw = {k: kw[k] for k in ("key_id2", "flow_start_s", "start_time", "end_time") if k in kw}
    okw.update({k: kw[k] for k in ("alpha", "eps", "min_samples") if kw.get(k)})      # 0 = the detector's default on both sides
    want = orc.run_job(algo, key, t, v, agg_flow=agg_flow, **okw)
    # every point, with verdicts (plotDF before the filter)
    allp = engine.run(algo, key, t, v, num_keys, agg_flow=agg_flow, emit_all=True, **kw)
    pk, pt, pv = want["points"]
    assert allp.n_rows == want["n_points"] == allp.stats["n_points"], (algo, "n_points", allp.n_rows, want["n_points"], allp.stats["n_points"])
    assert allp.stats["n_keys"] == want["n_keys"], (algo, "n_keys", allp.stats["n_keys"], want["n_keys"])
    assert (allp["key_id"] == pk).all() and (allp["flow_end_s"] == pt).all(), (algo, "every point", "key_id / flow_end_s")
    assert (allp["throughput"] == orc.u64_to_f64(pv)).all(), (algo, "every point", "throughput")          # integer aggregates, bit-exact
    n = np.diff(want["ptr"])
    assert (allp["stddev"] == np.repeat(want["sigma"], n)).all(), (algo, "every point", "stddev")       # same recurrence -> same bits
    assert (allp["algo_calc"] == want["calc_all"]).all(), (algo, "every point", "algo_calc")               # EWMA bit-exact / DBSCAN 0.0
    assert (allp["anomaly"].astype(bool) == want["anomaly_all"]).all(), (algo, "every point", "anomaly")
    assert allp.stats["n_anomalies"] == want["n_anomalies"], (algo, "n_anomalies", allp.stats["n_anomalies"], want["n_anomalies"])
    # the job's real output: anomalous points only
    res = engine.run(algo, key, t, v, num_keys, agg_flow=agg_flow, **kw)
    assert res.n_rows == want["n_anomalies"] == res.stats["n_anomalies"], (algo, "n_anomalies", res.n_rows, want["n_anomalies"], res.stats["n_anomalies"])
    for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
        assert (res[f] == want[f]).all(), (algo, "anomalous rows", f)
    return res, want


TOL = 1e-6   # BASELINE.json north_star: "EWMA/ARIMA scores within 1e-6 relative"


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.abs(b)


def assert_predictions(got, want, what):
    """every finite prediction within 1e-6 (in fact bit-identical); a fit whose optimiser walks into a non-finite
    likelihood yields NaN on both sides at the same index (Python: abs(x - nan) > sigma is False -> no anomaly row).
    That happens where the reference algorithm itself is numerically void: Box-Cox with a strongly negative lambda
    compresses the data to a variance of ~1e-18 next to the 1e6 diffuse prior, and P - K F K' cancels to a negative F
    (the scipy-driven restatement oracle/arima_oracle.py:calculate_arima shows the same NaNs at a similar rate)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaN predictions at different indices")
    inf = np.isinf(want)                  # inv_boxcox overflow (huge lambda): same infinity on both sides
    assert (got[inf] == want[inf]).all(), (what, "infinite predictions differ")
    fin = ~(nan | inf)
    rel = rel_err(got[fin], want[fin])
    assert (rel <= TOL).all(), (what, float(rel.max()), int((rel > TOL).sum()))
    assert (got[fin].view(np.uint64) == want[fin].view(np.uint64)).all(), (what, "within 1e-6 but not bit-identical", float(rel.max()))


CASES = [
    dict(agg_flow=""),
    dict(agg_flow="", start_time="2022-08-11 07:30:00", end_time="2022-08-11 08:00:00"),
    dict(agg_flow="", ns_ignore_list=["kube-system"]),
    dict(agg_flow="svc"),
    dict(agg_flow="svc", svc_port_name="svc-1:http", end_time="2022-08-11 08:00:00"),
    dict(agg_flow="external"),
    dict(agg_flow="external", external_ip="52.1.1.2"),
    dict(agg_flow="pod"),
    dict(agg_flow="pod", pod_label="APP1"),                       # ilike: case-insensitive
    dict(agg_flow="pod", pod_label="app_", pod_namespace="default"),   # '_' is a LIKE wildcard
    dict(agg_flow="pod", pod_name="pod-2"),
    dict(agg_flow="pod", pod_name="pod-2", pod_namespace="flow-visibility", ns_ignore_list=["kube-system"]),
    dict(agg_flow="pod", pod_name="pod-1", start_time="2022-08-11 07:50:00"),  # pod SQL ignores the time window
]


def canon(rows):
    return sorted(json.dumps(r, sort_keys=True) for r in rows)


class FakeResult:
    """Shaped like theia_amd.engine.TadResult, filled from the key-id oracle."""

    def __init__(self, want):
        self.n_rows = want["n_anomalies"]
        self._h = {k: want[k] for k in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev")}
        self.stats = {}

    def to_host(self):
        return self._h


def oracle_middle(prep, algo, agg_flow):
    return orc.run_job(algo, prep.key_id, prep.flow_end_s, prep.value, agg_flow=agg_flow, key_id2=prep.key_id2,
                       flow_start_s=prep.flow_start_s, start_time=prep.start_time, end_time=prep.end_time)


def lattice(t_live):
    """(t0, step, n_buckets) as the engine derives them from the live rows: the gcd lattice through the first and the last time"""
    t_live = np.asarray(t_live, dtype=np.int64)
    t0 = int(t_live.min())
    step = int(np.gcd.reduce(t_live - t0)) or 1
    return t0, step, (int(t_live.max()) - t0) // step + 1


def day_table(K, pts_per_key, rows_per_point, seed, span=86400):
    """second-resolution timestamps anywhere in a day (gcd 1), a few rows per (key, second)"""
    rng = np.random.default_rng(seed)
    P = K * pts_per_key
    pk = np.repeat(np.arange(K, dtype=np.uint64), pts_per_key)
    pt = 1660202814 + rng.integers(0, span, size=P).astype(np.int64)
    base = 1_000_000_000 + (orc.mix64(pk + np.uint64(3)) % np.uint64(3_000_000_000)).astype(np.int64)
    k = np.repeat(pk, rows_per_point)
    t = np.repeat(pt, rows_per_point)
    v = (np.repeat(base, rows_per_point) + rng.integers(-1_000_000, 1_000_000, size=k.size)).astype(np.uint64)
    spike = rng.random(k.size) < 2e-3
    v = np.where(spike, v * np.uint64(7), v)
    order = rng.permutation(k.size)
    return k[order], t[order], v[order]


def skewed_table(K, long_keys, long_len, seed, span=86400):
    """a few keys with a point at (almost) every second of a day, the rest with 1..12 points: the rank grid of the sparse path
    would be K x long_len cells for ~K * 6 points"""
    rng = np.random.default_rng(seed)
    n_k = rng.integers(1, 13, size=K)
    n_k[rng.choice(K, size=long_keys, replace=False)] = long_len
    n_k[rng.choice(K, size=K // 50, replace=False)] = 0          # keys without rows
    pk = np.repeat(np.arange(K, dtype=np.uint64), n_k)
    pt = np.concatenate([np.sort(rng.choice(span, size=n, replace=False)) for n in n_k]).astype(np.int64) + 1660202814
    base = 1_000_000_000 + (orc.mix64(pk + np.uint64(3)) % np.uint64(3_000_000_000)).astype(np.int64)
    v = (base + rng.integers(-1_000_000, 1_000_000, size=pk.size)).astype(np.uint64)
    v = np.where(rng.random(pk.size) < 3e-3, v * np.uint64(9), v)
    dup = rng.random(pk.size) < 0.2                                # some points have two rows
    k = np.concatenate([pk, pk[dup]]); t = np.concatenate([pt, pt[dup]]); v = np.concatenate([v, v[dup] // np.uint64(3)])
    order = rng.permutation(k.size)
    return k[order], t[order], v[order]


def class_boundary_table():
    """18 keys with a series at every class boundary (16 / 64 / 256 points), keys without points among them -> (key, t, value, K)"""
    rng = np.random.default_rng(3)
    n_k = np.array([0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 0, 5, 40], dtype=np.int64)
    K = n_k.size
    pk = np.repeat(np.arange(K, dtype=np.uint64), n_k)
    pt = np.concatenate([np.sort(rng.choice(5000, size=n, replace=False)) for n in n_k]).astype(np.int64) + 1660202814
    v = (2_000_000_000 + rng.integers(-3_000_000, 3_000_000, size=pk.size)).astype(np.uint64)
    v = np.where(rng.random(pk.size) < 0.02, v * np.uint64(5), v)
    order = rng.permutation(pk.size)
    return pk[order], pt[order], v[order], K


def check_lsd(engine, algo, k, t, v, K, agg_flow, paths=(4,), **kw):
    """the job on a sparse Stage 0 path against the oracle: every point with its verdict, then the anomalous rows; paths: the values of
    stats["stage0_path"] the plan in force may take (4: the LSD sort)"""
    want = orc.run_job(algo, k, t, v, agg_flow=agg_flow, **kw)
    allp = engine.run(algo, k, t, v, K, agg_flow=agg_flow, emit_all=True, **kw)
    assert allp.stats["stage0_path"] in paths, (algo, "stage0_path", allp.stats["stage0_path"], paths)
    pk, pt, pv = want["points"]
    if algo == "ARIMA":
        keep = np.repeat(np.array([r is not None for r in want["arima_results"]]), np.diff(want["ptr"]))
    else:
        keep = np.ones(pk.size, dtype=bool)
    assert allp.n_rows == int(keep.sum()), (algo, "every point", allp.n_rows, int(keep.sum()))
    assert (allp["key_id"] == pk[keep]).all() and (allp["flow_end_s"] == pt[keep]).all(), (algo, "every point", "key_id / flow_end_s")
    assert (allp["throughput"] == orc.u64_to_f64(pv)[keep]).all(), (algo, "every point", "throughput")
    assert (allp["stddev"] == np.repeat(want["sigma"], np.diff(want["ptr"]))[keep]).all(), (algo, "every point", "stddev")
    assert np.array_equal(allp["algo_calc"], want["calc_all"][keep], equal_nan=True), (algo, "every point", "algo_calc")
    assert (allp["anomaly"].astype(bool) == want["anomaly_all"][keep]).all(), (algo, "every point", "anomaly")
    res = engine.run(algo, k, t, v, K, agg_flow=agg_flow, **kw)
    assert res.stats["stage0_path"] in paths and res.n_rows == want["n_anomalies"], (algo, res.stats["stage0_path"], paths, res.n_rows, want["n_anomalies"])
    for f in ("key_id", "flow_end_s", "throughput", "stddev"):
        assert (res[f] == want[f]).all(), (algo, "anomalous rows", f)
    assert np.array_equal(res["algo_calc"], want["algo_calc"], equal_nan=True), (algo, "anomalous rows", "algo_calc")
    assert res.stats["n_keys"] == want["n_keys"] and res.stats["n_points"] == want["n_points"], (algo, res.stats, want["n_keys"], want["n_points"])
    return res, want


PART = dict(stage0="v2", sparse="always", sparse_sort="partition")


def check_part(engine, algo, k, t, v, K, agg_flow, paths=(8,), **kw):
    """check_lsd under the partition plan (path 8); its tests run no ARIMA job, for which alone the two checks ever differed"""
    return check_lsd(engine, algo, k, t, v, K, agg_flow, paths=paths, **kw)


PLANS = [
    dict(),
    dict(stage0="v1"),
    dict(stage0="v2", partition_pass="sort"),
    dict(stage0="v2", partition_pass="wc"),
    dict(stage0="v2", partition_pass="wc_sectors"),
    dict(stage0="v2", histogram="exact"),
    dict(stage0="v2", histogram="sampled"),
    dict(sparse="never"),
    dict(sparse="always", sparse_sort="lsd"),
    dict(stage0="v2", sparse="always", sparse_sort="partition"),
    dict(sparse="always", sparse_classes="always"),
]


def narrow_key(k):
    return None if k is None else np.where(k == SKIP64, SKIP32, k).astype(np.uint32)


@pytest.fixture
def plan(engine):
    def set_plan(**kw):
        engine.set_plan(**kw)
    yield set_plan
    engine.set_plan()


def e2e_flows(golden):
    """addFakeRecordforTAD (throughputanomalydetection_test.go:398-470): 90 rows of ONE connection, one per minute."""
    x = np.array(golden["throughput_list"], dtype=np.uint64)
    n = x.size
    const = lambda v: np.full(n, v)
    return {
        "flowStartSeconds": const(1660199214).astype(np.int64), "flowEndSeconds": (1660202814 + 60 * np.arange(n)).astype(np.int64),
        "sourceIP": const("10.10.1.25"), "destinationIP": const("10.10.1.33"), "sourceTransportPort": const(58076),
        "destinationTransportPort": const(5201), "protocolIdentifier": const(6),
        "sourcePodNamespace": const("test_namespace"), "sourcePodName": const("test_podName"),
        "destinationPodName": const("test_podName"), "destinationPodNamespace": const("test_namespace"),
        "sourcePodLabels": const("{test_key:test_value}"), "destinationPodLabels": const("{test_key:test_value}"),
        "destinationServicePortName": const("test_serviceportname"), "flowType": const(3), "throughput": x,
    }


def pandas_ids(cols, keep, cols_b=None, keep_b=None):
    """ids in order of first appearance over [kept rows of side a ++ kept rows of side b] (+ the first virtual rows)"""
    import pandas as pd
    n = len(cols[0])
    sides = [(cols, np.ones(n, bool) if keep is None else np.asarray(keep, bool), 0)]
    if cols_b is not None:
        sides.append((cols_b, np.ones(n, bool) if keep_b is None else np.asarray(keep_b, bool), 1))
    parts, vrows = [], []
    for cs, kp, side in sides:
        sel = np.flatnonzero(kp)
        parts.append([np.asarray(c)[sel] for c in cs] + [np.full(sel.size, side)])
        vrows.append(sel + side * n)
    cat = [np.concatenate([p[i] for p in parts]) for i in range(len(cols) + 1)]
    vrow = np.concatenate(vrows)
    if vrow.size == 0:
        return [np.full(n, SKIP) for _ in sides], np.zeros(0, np.uint64)
    codes, _ = pd.MultiIndex.from_arrays(cat).factorize()
    out, at = [], 0
    for cs, kp, side in sides:
        k = np.full(n, SKIP, dtype=np.uint64)
        m = int(kp.sum())
        k[np.flatnonzero(kp)] = codes[at:at + m].astype(np.uint64)
        at += m
        out.append(k)
    first = np.full(codes.max() + 1, -1, dtype=np.int64)
    for i in range(codes.size - 1, -1, -1):
        first[codes[i]] = vrow[i]
    return out, first.astype(np.uint64)


def _mix(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash8(words):
    """se_hash (tad_strbytes.h) of 8-byte strings given as little-endian uint64 words"""
    with np.errstate(over="ignore"):
        h = np.uint64(0x9E3779B97F4A7C15) ^ np.uint64(8)
        h = _mix(h ^ words) + np.uint64(0x632BE59BD9B4E019)
        return _mix(h)


def host(x):
    """a host or device array (or None) on the host"""
    return None if x is None else (x.to_host() if isinstance(x, DeviceArray) else np.asarray(x))


def column(strings, bits=32):
    """a list of bytes -> (offsets, data) in Arrow's layout"""
    off = np.zeros(len(strings) + 1, dtype=np.int32 if bits == 32 else np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return off, np.frombuffer(b"".join(strings), dtype=np.uint8).copy()


def device_column(engine, strings, bits=32, shift=0, validity=None, validity_offset=0):
    """the column in device memory, its bytes a slice starting `shift` bytes into an allocation; validity: one bool per row"""
    off, data = column(strings, bits)
    big = DeviceArray.from_host(engine, np.concatenate([np.full(shift, 0xEE, np.uint8), data, np.full(16, 0xEE, np.uint8)]))
    assert big.ptr % 16 == 0, ("device_column", big.ptr)
    col = [DeviceArray.from_host(engine, off), big.view(shift, data.size, np.uint8)]
    if validity is not None:
        bits_ = np.concatenate([np.ones(validity_offset, bool), np.asarray(validity, bool)])      # (the bits in front belong to other rows)
        col += [DeviceArray.from_host(engine, np.packbits(bits_, bitorder="little")), validity_offset]
    return tuple(col)


def exported(d, first=0, n=None):
    """the values a string dictionary holds (n of them from code `first` on), as a list of bytes"""
    off, data = d.export(first, n)
    assert off[0] == 0 and off.size >= 1, ("exported", off[:1], off.size)
    raw = data.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(off.size - 1)]


def keydict_snapshot(d):
    """what a key dictionary holds: (number of keys, copies of the exported columns, the side column)"""
    cols, side = d.export()
    return d.num_keys(), [c.copy() for c in cols], side.copy()


def assert_keydict_unchanged(d, snap, what=""):
    n, cols, side = keydict_snapshot(d)
    assert n == snap[0], (what, "num_keys", n, snap[0])
    assert all(np.array_equal(a, b) for a, b in zip(cols, snap[1])) and np.array_equal(side, snap[2]), (what, "columns")
