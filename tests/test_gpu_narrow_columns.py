"""GPU: narrow input columns (tad.h, TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32).  Every case runs the same seeded table twice — once in
8-byte columns (which the other GPU tests tie to the oracle) and once with 32-bit key and / or time columns — and requires the results
to be bit-identical, and the plan (stage0_path, hist_sampled) to be the same.  A few cases check the oracle directly."""
import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadError
from theia_amd import _capi as capi
from job_helpers import PLANS, SKIP64, narrow_key, plan  # noqa: F401  (plan: the fixture)

pytestmark = pytest.mark.gpu

FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev", "anomaly")
WIDTHS = ((32, 64), (64, 32), (32, 32))      # (key bits, time bits)


def table(seed, n, K, T, t0=1_700_000_000, step=60, skip=0.01, pod=False):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, K, n, dtype=np.uint64)
    k[rng.random(n) < skip] = SKIP64
    t = (t0 + step * rng.integers(0, T, n)).astype(np.int64)
    v = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    ts = (t - rng.integers(0, 4 * step, n)).astype(np.int64)
    k2 = None
    if pod:
        k2 = rng.integers(0, K, n, dtype=np.uint64)
        k2[rng.random(n) < 0.3] = SKIP64
    return dict(key_id=k, flow_end_s=t, value=v, key_id2=k2, flow_start_s=ts)


def columns(tab, kb, tb, device=False, with_start=False):
    """The table's columns at the given widths: numpy (host) or torch CUDA tensors (device)."""
    c = dict(tab)
    if not with_start:
        c["flow_start_s"] = None
    if kb == 32:
        c["key_id"], c["key_id2"] = narrow_key(c["key_id"]), narrow_key(c["key_id2"])
    if tb == 32:
        c["flow_end_s"] = c["flow_end_s"].astype(np.uint32)
        c["flow_start_s"] = None if c["flow_start_s"] is None else c["flow_start_s"].astype(np.uint32)
    if device:
        import torch
        def dev(a):
            if a is None:
                return None
            return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()
        c = {name: dev(a) for name, a in c.items()}
    return c


def same_result(a, b, what, same_plan=True):
    assert a.n_rows == b.n_rows, what
    for f in FIELDS:
        assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), (what, f)    # (ARIMA: a voided fit predicts NaN)
    plan = ("stage0_path", "hist_sampled") if same_plan else ()
    for s in ("rows_used", "n_keys", "n_points", "n_anomalies", "t0", "step", "n_buckets") + plan:
        assert a.stats[s] == b.stats[s], (what, s, a.stats[s], b.stats[s])


def run_both(engine, tab, K, algo="EWMA", widths=WIDTHS, device=False, with_start=False, agg_flow="svc", **kw):
    wide = engine.run(algo, num_keys=K, agg_flow=agg_flow, emit_all=True, **columns(tab, 64, 64, device, with_start), **kw)
    for kb, tb in widths:
        got = engine.run(algo, num_keys=K, agg_flow=agg_flow, emit_all=True, **columns(tab, kb, tb, device, with_start), **kw)
        same_result(wide, got, (algo, kb, tb, device))
    return wide


@pytest.mark.parametrize("p", PLANS, ids=lambda p: "-".join("%s=%s" % kv for kv in p.items()) or "auto")
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_stage0_strategy_is_bit_identical(engine, plan, p, device):
    plan(**p)
    tab = table(1, 300_001, 3000, 120)
    run_both(engine, tab, 3000, device=device)


@pytest.mark.parametrize("p", [dict(stage0="v1"), dict(stage0="v2", partition_pass="sort"), dict(stage0="v2", partition_pass="wc"),
                               dict(sparse="always", sparse_sort="lsd"), dict(stage0="v2", sparse="always", sparse_sort="partition")],
                         ids=["v1", "sort", "wc", "lsd", "sparse_partition"])
def test_pod_mode_and_start_time_windows(engine, plan, p):
    plan(**p)
    tab = table(2, 200_003, 1500, 90, pod=True)
    t0 = int(tab["flow_end_s"].min())
    run_both(engine, tab, 1500, agg_flow="pod", with_start=True, start_time=t0 + 600, end_time=t0 + 80 * 60)
    run_both(engine, tab, 1500, agg_flow="pod", device=True, with_start=True, start_time=t0 + 1200)


@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN", "ARIMA", "DROP"])
def test_every_detector(engine, algo):
    n, K, T = (20_000, 60, 40) if algo == "ARIMA" else (200_000, 2000, 100)
    tab = table(3, n, K, T)
    run_both(engine, tab, K, algo=algo, agg_flow="", device=True, widths=((32, 32),))
    run_both(engine, tab, K, algo=algo, agg_flow="svc", widths=((32, 64), (64, 32)))


@pytest.mark.parametrize("algo", ["EWMA", "DBSCAN"])
def test_narrow_columns_equal_the_oracle(engine, algo):
    tab = table(4, 100_000, 700, 80, pod=True)
    want = orc.run_job(algo, tab["key_id"], tab["flow_end_s"], tab["value"], agg_flow="pod", key_id2=tab["key_id2"])
    for device in (False, True):
        got = engine.run(algo, num_keys=700, agg_flow="pod", **columns(tab, 32, 32, device))
        assert got.n_rows == want["n_anomalies"]
        for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
            assert (got[f] == want[f]).all(), (algo, device, f)


@pytest.mark.parametrize("p", [dict(), dict(stage0="v2", partition_pass="wc"), dict(sparse="always", sparse_sort="lsd")], ids=["auto", "wc", "sparse"])
def test_aggregate_point_for_point(engine, plan, p):
    plan(**p)
    tab = table(5, 150_000, 1000, 64)
    wide = engine.aggregate(num_keys=1000, agg_flow="svc", **columns(tab, 64, 64))
    pk, pt, pv = orc.stage0(np.where(tab["key_id"] == SKIP64, SKIP64, tab["key_id"]), tab["flow_end_s"], tab["value"], "sum")
    assert np.array_equal(wide["key_id"], pk) and np.array_equal(wide["value"], pv)
    for kb, tb in WIDTHS:
        for device in (False, True):
            got = engine.aggregate(num_keys=1000, agg_flow="svc", **columns(tab, kb, tb, device))
            assert got.n_points == wide.n_points
            for f in ("key_id", "flow_end_s", "value"):
                assert np.array_equal(got[f], wide[f]), (kb, tb, device, f)
            assert got.stats["stage0_path"] == wide.stats["stage0_path"]


@pytest.mark.parametrize("p", [dict(), dict(sparse="always")], ids=["dense", "sparse"])
def test_stream_batch_by_batch(engine, plan, p):
    plan(**p)
    K, T = 800, 90
    tab = table(6, 120_000, K, T)
    bucket = (tab["flow_end_s"] - tab["flow_end_s"].min()) // 60
    states = {}
    for kb, tb in ((64, 64),) + WIDTHS:
        st = engine.state_create(K)
        rows = []
        for lo, hi in ((0, 30), (30, 31), (31, T)):
            sel = (bucket >= lo) & (bucket < hi)
            sub = {name: (None if a is None else a[sel]) for name, a in tab.items()}
            c = columns(sub, kb, tb, device=(kb == 32 and tb == 32))
            r = engine.run_stream(st, c["key_id"], c["flow_end_s"], c["value"], agg_flow="svc", emit_all=True)
            rows.append({f: r[f] for f in FIELDS})
        states[(kb, tb)] = (st.export(), rows)
        st.close()
    want_state, want_rows = states[(64, 64)]
    for w in WIDTHS:
        got_state, got_rows = states[w]
        for f in want_state:
            assert np.array_equal(got_state[f], want_state[f]), (w, f)
        for a, b in zip(got_rows, want_rows):
            for f in FIELDS:
                assert np.array_equal(a[f], b[f]), (w, f)


@pytest.mark.parametrize("p", [dict(stage0="v1"), dict(stage0="v2", partition_pass="wc"), dict(sparse="always")], ids=["v1", "wc", "sparse"])
def test_times_beyond_2_31_are_zero_extended(engine, plan, p):
    plan(**p)
    tab = table(7, 100_000, 500, 50, t0=3_000_000_000)
    wide = run_both(engine, tab, 500, widths=((64, 32), (32, 32)))
    assert wide["flow_end_s"].min() >= 3_000_000_000
    import torch      # an int32 tensor is read as the UInt32 bits of a DateTime
    t = torch.from_numpy(tab["flow_end_s"].astype(np.uint32).view(np.int32)).cuda()
    assert int(t.min()) < 0
    k = torch.from_numpy(tab["key_id"].view(np.int64)).cuda()
    v = torch.from_numpy(tab["value"].view(np.int64)).cuda()
    same_result(wide, engine.run("EWMA", k, t, v, 500, agg_flow="svc", emit_all=True), "int32 tensor")


def test_skip32_rows_do_not_take_part(engine):
    tab = table(8, 50_000, 300, 40, skip=0.4, pod=True)
    wide = run_both(engine, tab, 300, agg_flow="pod")
    assert wide.stats["rows_used"] < 2 * 50_000 * 0.8


@pytest.mark.parametrize("p", [dict(stage0="v1"), dict(stage0="v2", partition_pass="wc"), dict(sparse="always")], ids=["v1", "wc", "sparse"])
def test_bad_keys_and_key_spaces(engine, plan, p):
    plan(**p)
    tab = table(9, 40_000, 300, 40)
    tab["key_id"][123] = 300                 # = num_keys
    with pytest.raises(TadError) as wide:
        engine.run("EWMA", num_keys=300, agg_flow="svc", **columns(tab, 64, 64))
    with pytest.raises(TadError) as narrow:
        engine.run("EWMA", num_keys=300, agg_flow="svc", **columns(tab, 32, 32))
    assert wide.value.code == narrow.value.code == capi.TAD_ERR_KEY_RANGE
    tab = table(9, 1000, 300, 40)
    for K in ((1 << 32) - 1, 1 << 40):
        with pytest.raises(TadError) as e:
            engine.run("EWMA", num_keys=K, agg_flow="svc", **columns(tab, 32, 64))
        assert e.value.code == capi.TAD_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("p", [dict(stage0="v1"), dict(stage0="v2", partition_pass="wc"), dict(stage0="v2", partition_pass="sort"),
                               dict(sparse="always", sparse_sort="lsd")], ids=["v1", "wc", "sort", "lsd"])
def test_unaligned_device_columns_and_ragged_row_counts(engine, plan, p, off):
    import torch
    plan(**p)
    n = 100_003 + off
    tab = table(10 + off, n, 900, 70, pod=True)
    wide = engine.run("EWMA", num_keys=900, agg_flow="pod", emit_all=True, **columns(tab, 64, 64, device=True))
    for kb, tb in WIDTHS:
        c = columns(tab, kb, tb)
        shifted = {}
        for name, a in c.items():
            if a is None:
                continue
            buf = torch.zeros(n + off, dtype={8: torch.int64, 4: torch.int32}[a.dtype.itemsize], device="cuda")
            buf[off:] = torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()
            shifted[name] = buf[off:]
        torch.cuda.synchronize()     # (the copies ran on torch's stream; the engine reads on its own)
        got = engine.run("EWMA", num_keys=900, agg_flow="pod", emit_all=True, **shifted)
        same_result(wide, got, (kb, tb, off), same_plan=False)   # (an unaligned column takes the row-by-row pass B: another plan, same rows)


def test_full_size_c2_table():
    """BASELINE.json's C2 table (1e8 rows / 1e5 keys / 250 buckets; its synthetic times fit 32 bits) at (32, 32) equals the 8-byte run,
    on a fresh engine as a controller's job meets it."""
    import torch
    from theia_amd import TadEngine
    engine = TadEngine(device=0)
    n, K, T = 100_000_000, 100_000, 250
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    v = torch.empty(n, dtype=torch.int64, device="cuda")
    engine.synth(0, n, K, T, into=(k, t, v))
    assert int(t.max()) < (1 << 32) and int(t.min()) >= 0
    wide = engine.run("EWMA", k, t, v, K, agg_flow="svc")
    k32, t32 = k.to(torch.int32), t.to(torch.int32)
    torch.cuda.synchronize()         # (the narrowing ran on torch's stream; the engine reads on its own)
    got = engine.run("EWMA", k32, t32, v, K, agg_flow="svc")
    assert got.n_rows == wide.n_rows > 0
    for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
        assert np.array_equal(got[f], wide[f]), f
    for s in ("rows_used", "n_points", "stage0_path", "hist_sampled"):
        assert got.stats[s] == wide.stats[s], s
    engine.close()
