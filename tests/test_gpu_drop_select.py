"""GPU: the drop job's flow-row query (tad_drop_select, include/tad.h) and the two jobs that start from it.  Every output column and the
row order are compared bit for bit with the direct numpy form of the row rule in tests/drop_query_ref.py; the end-to-end case holds
drop_detection_from_flows and PeriodicalDropDetection.feed_flows against the pandas restatement of the query, oracle/drop_oracle.py and
the existing count-fed paths.  The kernels' geometry is mirrored in the two constants below."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drop_query_ref as dq  # noqa: E402
from oracle import drop_oracle as dro  # noqa: E402
from theia_amd import TadError, _capi  # noqa: E402
from theia_amd.engine import DeviceArray  # noqa: E402
from stream_helpers import DAY0, N_DAYS, N_ENDPOINTS, PLANTED, SHORT, counts_of, flow_table, flows, keyed  # noqa: F401  (flows: the fixture)

pytestmark = pytest.mark.gpu

LANE_ROWS = 16        # kDselLaneRows
TILE_ROWS = 4096      # kDselTileRows
WAVE_ROWS = 64 * LANE_ROWS
CODES = ("src_ip", "src_pod_ns", "src_pod_name", "dst_ip", "dst_pod_ns", "dst_pod_name")


def dev(engine, a, offset=0):
    """a device copy of `a` that starts `offset` bytes into its buffer (hipMalloc aligns the buffer itself to 256 bytes)"""
    a = np.ascontiguousarray(a)
    buf = DeviceArray(engine, offset + a.nbytes + 32, np.uint8)
    assert buf.ptr % 256 == 0
    if a.nbytes:
        engine._check(engine._lib.tad_copy_to_device(engine._h, buf.ptr + offset, a.ctypes.data, a.nbytes))
    return buf.view(offset, a.size, a.dtype)


def select(engine, c, device=True, out="device", offsets=None, keep=None, null=(0, 0), **kw):
    offsets = offsets or {}
    put = (lambda name, a: dev(engine, a, offsets.get(name, 0))) if device else (lambda name, a: a)
    cols = {name: put(name, c[name]) for name in ("ingress_action", "egress_action", "flow_start_s", "flow_end_s") + CODES if c.get(name) is not None}
    if keep is not None:
        keep = put("keep", np.asarray(keep, dtype=np.uint8))
    rows = engine.drop_select(cols["ingress_action"], cols["egress_action"], cols["flow_start_s"], *[cols[k] for k in CODES], flow_end_s=cols.get("flow_end_s"),
                              src_pod_null=null[0], dst_pod_null=null[1], keep=keep, out=out, **kw)
    assert rows.memory == out
    for name, col in zip(dq.OUT_FIELDS, rows):
        assert isinstance(col, DeviceArray if out == "device" else np.ndarray), name
    return rows.to_host()


def reference(c, keep=None, null=(0, 0), **kw):
    return dq.select_rows(c["ingress_action"], c["egress_action"], c["flow_start_s"], *[c[k] for k in CODES], flow_end_s=c.get("flow_end_s"),
                          src_pod_null=null[0], dst_pod_null=null[1], keep=keep, **kw)


def assert_columns(got, want, what=""):
    assert list(got) == list(dq.OUT_FIELDS)
    for f in dq.OUT_FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f)


def check(engine, c, **kw):
    got, want = select(engine, c, **{k: v for k, v in kw.items()}), reference(c, **{k: v for k, v in kw.items() if k not in ("device", "out", "offsets")})
    assert_columns(got, want, str(sorted(kw)))
    return want


# ---- geometry ----
SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 5]
PATTERNS = ["none", "all", "first", "last", "tile_edges", "wave_edges", "r64", "r2"]


def pattern(name, n):
    s = np.zeros(n, dtype=bool)
    if name == "all":
        s[:] = True
    elif name == "first":
        s[:1] = True
    elif name == "last":
        s[n - 1:] = True
    elif name in ("tile_edges", "wave_edges"):
        step = TILE_ROWS if name == "tile_edges" else WAVE_ROWS
        for b in range(step, n, step):
            s[b - 1] = s[b] = True
    elif name in ("r64", "r2"):
        s = np.random.default_rng(n).random(n) < (1 / 64 if name == "r64" else 0.5)
    return s


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_selection_pattern(engine, n, name):
    s = pattern(name, n)
    # from the mirror, before the engine is asked: the pattern puts a selected row on each edge it names
    lane, tile = np.arange(n) // LANE_ROWS % 64, np.arange(n) // TILE_ROWS
    if name == "tile_edges":
        for t in range(1, (n + TILE_ROWS - 1) // TILE_ROWS):
            assert s[t * TILE_ROWS - 1] and s[t * TILE_ROWS] and tile[t * TILE_ROWS - 1] == t - 1 and tile[t * TILE_ROWS] == t
        assert s.sum() == 2 * ((n - 1) // TILE_ROWS if n else 0)
    if name == "wave_edges":
        for b in range(WAVE_ROWS, n, WAVE_ROWS):
            assert s[b - 1] and s[b] and lane[b - 1] == 63 and lane[b] == 0
        assert s.sum() == 2 * ((n - 1) // WAVE_ROWS if n else 0)
    if name == "first" and n:
        assert s[0] and s.sum() == 1
    if name == "last" and n:
        assert s[n - 1] and s.sum() == 1
    c = flow_table(n, s, seed=n)
    want = check(engine, c)
    assert np.array_equal(want["row"], np.flatnonzero(s).astype(np.uint64))


# ---- alignment ----
@pytest.mark.parametrize("offs", [(1, 3, 8), (3, 8, 15), (8, 15, 1), (15, 1, 3), (1, 1, 1), (0, 15, 0)])
def test_action_and_keep_columns_that_are_device_slices(engine, offs):
    n = 2 * TILE_ROWS + 37
    c = flow_table(n, pattern("r2", n), seed=7)
    keep = np.random.default_rng(5).random(n) < 0.7
    offsets = {"ingress_action": offs[0], "egress_action": offs[1], "keep": offs[2]}
    check(engine, c, offsets=offsets, keep=keep)
    check(engine, c, offsets=offsets)


def test_eight_byte_columns_that_are_only_eight_byte_aligned(engine):
    n = TILE_ROWS + 19
    c = flow_table(n, pattern("r2", n), seed=8)
    check(engine, c, offsets={k: 8 for k in CODES + ("flow_start_s", "flow_end_s")}, start_time=DAY0 + 3 * dq.DAY, end_time=DAY0 + 15 * dq.DAY)


def test_u32_time_columns_that_are_only_four_byte_aligned(engine):
    n = TILE_ROWS + 19
    c = flow_table(n, pattern("r2", n), seed=9)
    c["flow_start_s"], c["flow_end_s"] = c["flow_start_s"].astype(np.uint32), c["flow_end_s"].astype(np.uint32)
    for off in (4, 12):
        check(engine, c, offsets={"flow_start_s": off, "flow_end_s": off}, start_time=DAY0 + 3 * dq.DAY, end_time=DAY0 + 15 * dq.DAY)


# ---- the row rule ----
def test_every_pair_of_actions(engine):
    acts = (0, 1, 2, 3, 4, 255)
    pairs = np.array([(a, b) for a in acts for b in acts] * 5, dtype=np.uint8)
    n = len(pairs)
    c = flow_table(n, np.zeros(n, bool), seed=11)
    c["ingress_action"], c["egress_action"] = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    want = check(engine, c)
    ia, ea = pairs[:, 0].astype(int), pairs[:, 1].astype(int)
    drops = lambda a: (a == 2) | (a == 3)
    assert np.array_equal(want["row"], np.flatnonzero(drops(ia) | drops(ea)).astype(np.uint64)) and want["row"].size == 5 * 20
    assert np.array_equal(want["direction"], np.where(drops(ia[want["row"].astype(int)]), 0, 1))         # ingress wins when both drop
    assert (drops(ia) & drops(ea)).sum() == 5 * 4


@pytest.mark.parametrize("null", [(0, 0), (-1, -1), (0, 7), (7, -1)], ids=["present", "none", "differ", "one-side"])
def test_pod_null_codes(engine, null):
    n = 3000
    c = flow_table(n, pattern("r2", n), seed=12)
    want = check(engine, c, null=null)
    row, ing = want["row"].astype(int), want["direction"] == 0
    pod = np.where(ing, c["dst_pod_name"][row], c["src_pod_name"][row])
    assert np.array_equal(want["endpoint_kind"] == 0, pod == np.where(ing, null[1], null[0]))
    if null == (-1, -1):
        assert want["endpoint_kind"].all()
    else:
        assert 0 < want["endpoint_kind"].sum() < row.size


def test_an_endpoint_seen_as_pod_in_one_row_and_as_ip_in_another(engine):
    c = flow_table(4, np.ones(4, bool), seed=13)
    c["ingress_action"][:], c["egress_action"][:] = 2, 0
    c["dst_ip"][:], c["dst_pod_ns"][:] = 9, 3
    c["dst_pod_name"][:] = [9, 0, 9, 0]            # the pod's name code equals the IP's code: only the kind column tells them apart
    want = check(engine, c)
    assert want["endpoint_kind"].tolist() == [1, 0, 1, 0] and want["endpoint_name"].tolist() == [9, 9, 9, 9] and want["endpoint_ns"].tolist() == [3, 0, 3, 0]


# ---- times ----
def test_start_is_inclusive_and_end_exclusive_at_the_exact_second(engine):
    S, E = DAY0 + 5000, DAY0 + 90000
    ts = np.array([S - 1, S, S + 1, S + 10, S + 10, S + 10, S - 1, S], dtype=np.int64)
    te = np.array([E - 5, E - 5, E - 5, E - 1, E, E + 1, E, E - 1], dtype=np.int64)
    c = flow_table(ts.size, np.ones(ts.size, bool), seed=14)
    c["flow_start_s"], c["flow_end_s"] = ts, te
    want = check(engine, c, start_time=S, end_time=E)
    assert want["row"].tolist() == [1, 2, 3, 7]
    assert check(engine, c, start_time=S)["row"].tolist() == [1, 2, 3, 4, 5, 7]
    assert check(engine, c, end_time=E)["row"].tolist() == [0, 1, 2, 3, 7]
    c32 = dict(c, flow_start_s=ts.astype(np.uint32), flow_end_s=te.astype(np.uint32))
    assert check(engine, c32, start_time=S, end_time=E)["row"].tolist() == [1, 2, 3, 7]


@pytest.mark.parametrize("which", ["start", "end", "keep"])
def test_a_filter_removes_a_row_the_action_mask_kept_at_each_tile_edge(engine, which):
    n = 3 * TILE_ROWS + 5
    c = flow_table(n, np.ones(n, bool), seed=15)
    edge = pattern("tile_edges", n)
    assert edge.sum() == 6 and all(edge[t * TILE_ROWS - 1] and edge[t * TILE_ROWS] for t in (1, 2, 3))
    S, E = DAY0 + 2 * dq.DAY, DAY0 + 30 * dq.DAY
    c["flow_start_s"] = np.where(edge, S - 1, S + np.arange(n)) if which == "start" else S + np.arange(n)
    c["flow_end_s"] = np.where(edge, E, E - 1) if which == "end" else np.full(n, E - 1)
    kw = {"keep": ~edge} if which == "keep" else {"start_time": S, "end_time": E}
    want = check(engine, c, **kw)
    assert np.array_equal(want["row"], np.flatnonzero(~edge).astype(np.uint64))


def test_the_day_is_the_floor_of_the_start(engine):
    ts = np.array([86399, 86400, 86401, -1, -86400, -86401, 0, DAY0 - 1, DAY0], dtype=np.int64)
    c = flow_table(ts.size, np.ones(ts.size, bool), seed=16)
    c["flow_start_s"], c["flow_end_s"] = ts, ts + 5
    want = check(engine, c)
    assert want["day_s"].tolist() == [0, 86400, 86400, -86400, -86400, -2 * 86400, 0, DAY0 - 86400, DAY0]


def test_u32_times_are_zero_extended(engine):
    ts = np.array([2 ** 31, 4000000000, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.uint32)
    c = flow_table(ts.size, np.ones(ts.size, bool), seed=17)
    c["flow_start_s"], c["flow_end_s"] = ts, ts
    want = check(engine, c, start_time=2 ** 31 - 1, end_time=2 ** 32)
    assert want["day_s"].tolist() == [int(t) // 86400 * 86400 for t in ts.tolist()] and want["day_s"].min() > 0
    assert check(engine, c, start_time=2 ** 31 + 1)["row"].tolist() == [1, 3]


# ---- the call ----
def test_keep_combines_with_the_actions(engine):
    n = TILE_ROWS + 100
    c = flow_table(n, pattern("r2", n), seed=18)
    keep = (np.arange(n) % 3 != 0).astype(np.uint8) * np.uint8(255)           # any non-zero byte keeps
    want = check(engine, c, keep=keep)
    assert 0 < want["row"].size < pattern("r2", n).sum() and np.all(want["row"] % 3 != 0)
    assert check(engine, c, keep=np.zeros(n, np.uint8))["row"].size == 0


def test_host_and_device_inputs_and_outputs_agree_and_a_call_repeats(engine):
    n = 2 * TILE_ROWS + 11
    c = flow_table(n, pattern("r64", n), seed=19)
    keep = np.random.default_rng(3).random(n) < 0.9
    kw = dict(keep=keep, start_time=DAY0 + dq.DAY, end_time=DAY0 + 19 * dq.DAY)
    want = reference(c, **kw)
    assert want["row"].size > 20
    for device in (True, False):
        for out in ("device", "host"):
            assert_columns(select(engine, c, device=device, out=out, **kw), want, "%s %s" % (device, out))
    cols = {k: dev(engine, v) for k, v in c.items()}
    dkeep = dev(engine, keep.astype(np.uint8))
    call = lambda: engine.drop_select(cols["ingress_action"], cols["egress_action"], cols["flow_start_s"], *[cols[k] for k in CODES],
                                      flow_end_s=cols["flow_end_s"], src_pod_null=0, dst_pod_null=0, keep=dkeep, start_time=kw["start_time"], end_time=kw["end_time"])
    a, b = call(), call()                      # the same call twice: the inputs are only read
    assert_columns(a.to_host(), want)
    assert_columns(b.to_host(), want)
    for k, v in c.items():
        assert np.array_equal(cols[k].to_host(), v), k
    a.close()
    assert_columns(b.to_host(), want)          # one result does not live in the other


def test_every_refusal_leaves_no_result_and_a_message(engine):
    lib, n = engine._lib, 64
    c = flow_table(n, np.ones(n, bool), seed=20)
    keepalive = {k: np.ascontiguousarray(v) for k, v in c.items()}
    full = {k: v.ctypes.data for k, v in keepalive.items()}

    def call(start=0, end=0, flags=0, **override):
        fc = _capi.DropFlowColumns(n_rows=n, src_pod_null=-1, dst_pod_null=-1, flags=flags, memory=_capi.TAD_MEM_HOST)
        for k, v in dict(full, **override).items():
            setattr(fc, k, v)
        res = ctypes.POINTER(_capi.DropRows)()
        rc = lib.tad_drop_select(engine._h, ctypes.byref(fc), start, end, _capi.TAD_MEM_HOST, ctypes.byref(res))
        return rc, res, (lib.tad_last_error(engine._h) or b"").decode()

    rc, res, _ = call()
    assert rc == _capi.TAD_OK and res and res.contents.n_rows == n
    lib.tad_drop_rows_free(engine._h, res)
    for name in ("ingress_action", "egress_action", "flow_start_s") + CODES:
        rc, res, msg = call(**{name: None})
        assert rc == _capi.TAD_ERR_INVALID_ARGUMENT and not res and "tad_drop_select" in msg, name
    rc, res, msg = call(end=DAY0, flow_end_s=None)
    assert rc == _capi.TAD_ERR_INVALID_ARGUMENT and not res and "flow_end_s" in msg
    rc, res, _ = call(flow_end_s=None)         # without an end bound the column is optional
    assert rc == _capi.TAD_OK and res.contents.n_rows == n
    lib.tad_drop_rows_free(engine._h, res)
    for flags in (_capi.TAD_FLAG_EMIT_ALL_POINTS, _capi.TAD_FLAG_KEY_U32, _capi.TAD_FLAG_TIME_U32 | 8, 1 << 31):
        rc, res, msg = call(flags=flags)
        assert rc == _capi.TAD_ERR_INVALID_ARGUMENT and not res and "TAD_FLAG_TIME_U32" in msg, flags
    res = ctypes.POINTER(_capi.DropRows)()
    fc = _capi.DropFlowColumns(n_rows=n)
    assert lib.tad_drop_select(None, ctypes.byref(fc), 0, 0, _capi.TAD_MEM_HOST, ctypes.byref(res)) == _capi.TAD_ERR_INVALID_ARGUMENT and not res
    assert b"engine is NULL" in lib.tad_last_error(None)
    # no rows: an empty result, whatever the pointers
    fc = _capi.DropFlowColumns(n_rows=0)
    assert lib.tad_drop_select(engine._h, ctypes.byref(fc), 0, 0, _capi.TAD_MEM_DEVICE, ctypes.byref(res)) == _capi.TAD_OK and res and res.contents.n_rows == 0
    lib.tad_drop_rows_free(engine._h, res)
    with pytest.raises(TadError):
        engine.drop_select(c["ingress_action"], c["egress_action"][:-1], c["flow_start_s"], *[c[k] for k in CODES])


# ---- end to end: flow rows -> result rows ----
# Why 20 days: with one outlier among n otherwise equal points, |x - mean| / std = (n - 1) / sqrt(n), which exceeds 3 only from n = 11 on


def test_flow_rows_to_result_rows(engine, flows):
    import pandas as pd
    from theia_amd import drop_detection as dd
    c, d = flows["cols"], flows["dict"]
    _, want = counts_of(flows)
    assert int(want["dropNumber"].sum()) == flows["m"] and len(want) == (N_ENDPOINTS - len(SHORT)) * N_DAYS + 2 * len(SHORT)
    # preconditions, on the CPU: the oracle over the pandas counts finds every planted day, not every day, and nothing for the two-day endpoints
    codes, uniq = pd.MultiIndex.from_arrays([want["endpoint"], want["direction"]]).factorize()
    day = np.asarray(pd.to_datetime(want["date"]).values.astype("datetime64[D]").astype(np.int64))
    o = dro.run_job(codes.astype(np.uint64), day, want["dropNumber"].to_numpy().astype(np.uint64))
    oracle = sorted((uniq[int(k)][0], uniq[int(k)][1], float(a).hex(), float(s).hex(), str(np.datetime64(int(t), "D")), int(x))
                    for k, t, x, a, s in zip(o["key_id"], o["flow_end_s"], o["throughput"], o["algo_calc"], o["stddev"]))
    found = {(r[0], r[1]): r[4] for r in oracle if r[5] == 60}
    assert found == flows["planted"] and len(found) == len(PLANTED)
    assert 0 < len(oracle) < len(want) and o["keys_no_result"] == len(SHORT)
    assert not {(r[0], r[1]) for r in oracle} & set(flows["short"])
    # 1: the device path returns exactly the oracle's rows
    got = dd.drop_detection_from_flows(engine, c, d, detection_id="t")
    assert keyed(got) == oracle
    assert all(r[0] == "initial" and r[1] == "t" for r in got)
    # ... also from device-resident columns
    on_device = {k: dev(engine, v) for k, v in c.items()}
    assert keyed(dd.drop_detection_from_flows(engine, on_device, d)) == oracle
    # 2: and the rows of the existing count-fed job
    assert keyed(got) == keyed(dd.drop_detection_table(want["endpoint"], want["direction"], want["date"], want["dropNumber"], engine=engine))
    # 3: four five-day feeds of flow rows against the same feeds of counts
    by_flows, by_counts = dd.PeriodicalDropDetection(engine), dd.PeriodicalDropDetection(engine)
    total = 0
    for f in range(4):
        part, cnt = counts_of(flows, 5 * f, 5 * f + 5)
        a = by_flows.feed_flows(part, d, detection_id="p")
        b = by_counts.feed(cnt["endpoint"], cnt["direction"], cnt["date"], cnt["dropNumber"], detection_id="p")
        assert keyed(a) == keyed(b), f
        assert all(r[0] == "periodical" for r in a)
        total += len(a)
    assert total > 0
    assert keyed(by_flows.window()) == keyed(by_counts.window())
    with pytest.raises(TadError):                # a day split over two feeds is a late row: refused
        by_flows.feed_flows(counts_of(flows, 19, 20)[0], d)
