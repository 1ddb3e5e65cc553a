"""GPU: the detectors' parameters away from their defaults, against the CPU oracle bit for bit.

tad_job's ewma_alpha, dbscan_eps and dbscan_min_samples are 0 (= default) in every other whole-job parity test.  At the default
alpha 0.5 both products of e = (1 - alpha) * e + alpha * x are exact and 1 - alpha == alpha: a recurrence with the two swapped, with
0.5 hard-coded, with a fused multiply-add or with a float32 alpha gives the same bits (tests/test_oracle_parameters.py shows it on
the CPU, and shows that at the alphas used here every one of them leaves the oracle's bits).  The default eps and min_samples put
about 2 % of the synthetic keys on the DBSCAN work list; the pairs used here list every key, no key, more keys than the tile
pass's contiguous series hold (compact_cap), make every point noise and use an eps that is no integer — each regime asserted from
the oracle alone before the GPU is asked.

Every EWMA site is reached: the lane and the wavefront-per-key form of the sigma / count walk and of the emit, the staged emit, the
series entry points, the sparse forms and both stream kernels."""
import numpy as np
import pytest

from oracle import stream_oracle as so
from oracle import tad_oracle as orc
from job_helpers import check_job, class_boundary_table, day_table

pytestmark = pytest.mark.gpu

ALPHAS = (0.3, 1 / 3, 0.05, 0.9, 1.0)
K_P, N_POINTS_P = 9000, 241_163
K_DAY = 3000
LSD = dict(sparse="always", sparse_sort="lsd")
PARTITION = dict(stage0="v2", sparse="always", sparse_sort="partition")
CLASSES = dict(sparse="always", sparse_sort="lsd", sparse_classes="always")
CLASSES_PARTITION = dict(stage0="v2", sparse="always", sparse_sort="partition", sparse_classes="always")
SPARSE_FORMS = {"lsd": (LSD, 4), "partition": (PARTITION, 8), "classes": (CLASSES, 6), "classes_partition": (CLASSES_PARTITION, 9)}     # plan, stage0_path


@pytest.fixture(autouse=True, params=["v1", "v2", "v2wc"])
def stage0(request, engine):
    """Every test runs with every Stage-0 strategy, as in tests/test_gpu_parity.py: v1 = direct atomic scatter, v2 = partition + LDS
    tiles with the sort-by-tile partition pass, v2wc = v2 with the write-combining partition pass."""
    engine.set_plan(stage0=request.param[:2], partition_pass="wc" if request.param == "v2wc" else "sort")
    yield request.param
    engine.set_plan()


@pytest.fixture(scope="module")
def P():
    """9000 keys with series of 16 to 37 points: 241 163 points from 400 000 rows"""
    return orc.synth_rows(0, 400_000, K_P, 40)


@pytest.fixture(scope="module")
def day():
    """3000 keys with 20 points each at any second of a day (the table of test_day_of_seconds_through_the_partition_pass): sparse"""
    return day_table(K_DAY, 20, 3, seed=21)


@pytest.fixture(scope="module")
def classes():
    """(key, t, value, K) of test_length_classes_forced_small_tables: a series at every boundary of the length classes"""
    return class_boundary_table()


@pytest.fixture(scope="module")
def few_long_keys():
    """(K, T) = (3, 700) and (70, 1300), built as in test_job_long_series_on_few_keys_wavefront_per_key: a wavefront per key; a fifth
    of the cells absent, key 1 with a single point"""
    def build(K, T):
        k, t, v = orc.synth_rows(11, 40 * K * T // 10, K, T)
        keep = (orc.mix64(k * np.uint64(977) + t.astype(np.uint64)) % np.uint64(5)) != 0
        keep &= ~((k == 1) & (t != t.min()))
        return k[keep], t[keep], v[keep]
    return {(K, T): build(K, T) for K, T in ((3, 700), (70, 1300))}


@pytest.fixture(scope="module", autouse=True)
def oracle_once():
    """check_job asks the oracle for the job it compares with; the three Stage-0 strategies and the emit plans ask for the same jobs.
    The oracle runs once per (table, detector, parameters): the module's tables are module-scoped fixtures, so the identity of the
    key column names the table.  The results are read, never written."""
    real, memo = orc.run_job, {}

    def run_job(algo, key_id, flow_end_s, value, **kw):
        try:
            tag = (algo, id(key_id), id(value)) + tuple(sorted(kw.items()))
            hash(tag)
        except (TypeError, ValueError):     # a column among the arguments: not one of this module's shared jobs
            return real(algo, key_id, flow_end_s, value, **kw)
        if tag not in memo:
            memo[tag] = (real(algo, key_id, flow_end_s, value, **kw), key_id, value)      # (the columns stay alive: ids are not reused)
        return memo[tag][0]
    orc.run_job = run_job
    yield
    orc.run_job = real


# ------------------------------------------------------------------ B1: the EWMA job
EWMA_ANOMALIES_P = {(0.3, "svc"): 44_801, (1 / 3, "svc"): 41_503, (0.05, "svc"): 106_086, (0.3, ""): 194_521, (0.9, "svc"): 0, (1.0, "svc"): 0}


@pytest.mark.parametrize("emit_plan", [{}, {"ewma_emit_rows": 64}, {"ewma_emit": "lane"}], ids=["staged", "staged_64_rows", "lane"])
@pytest.mark.parametrize("agg", ["svc", ""], ids=["sum", "max"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_ewma_job_alpha(engine, stage0, P, alpha, agg, emit_plan):
    """k_key_sigma<EWMA_COUNT> and the emit kernels (staged with the default capacity, staged with one row per key so that most rows
    overflow, lane per key) at five alphas.  alpha 0.9 and 1.0 flag next to nothing on sums: there the emit_all leg of check_job
    carries the comparison of every point's EWMA value."""
    k, t, v = P
    with engine.plan(**emit_plan):
        res, want = check_job(engine, "EWMA", k, t, v, K_P, agg_flow=agg, alpha=alpha)
    assert want["n_points"] == N_POINTS_P and want["n_keys"] == K_P
    if alpha not in (0.9, 1.0):
        assert want["n_anomalies"] > 1000
    if (alpha, agg) in EWMA_ANOMALIES_P:
        assert want["n_anomalies"] == EWMA_ANOMALIES_P[alpha, agg]
    assert res.stats["stage0_path"] in {"v1": (1,), "v2": (2,), "v2wc": (2, 3)}[stage0]


@pytest.mark.parametrize("alpha", ALPHAS)
def test_ewma_job_alpha_wavefront_per_key(engine, few_long_keys, alpha):
    """T >= 512 buckets on few keys: the wavefront-per-key forms of the sigma / count walk and of the emit"""
    k, t, v = few_long_keys[3, 700]
    res, want = check_job(engine, "EWMA", k, t, v, 3, agg_flow="svc", alpha=alpha)
    assert res.stats["n_buckets"] >= 512 and want["n_points"] > 1000
    if alpha not in (0.9, 1.0):
        assert want["n_anomalies"] > 0


@pytest.mark.parametrize("form", list(SPARSE_FORMS))
@pytest.mark.parametrize("alpha", ALPHAS)
def test_ewma_job_alpha_sparse_forms(engine, stage0, day, classes, alpha, form):
    """the sparse Stage 0 (LSD sort, partition pass + LDS sorts) and the length classes walk the points with the same recurrence"""
    plan, path = SPARSE_FORMS[form]
    k, t, v, K = classes if form.startswith("classes") else day + (K_DAY,)
    with engine.plan(**plan):
        res, want = check_job(engine, "EWMA", k, t, v, K, agg_flow="svc", alpha=alpha)
        allp = engine.run("EWMA", k, t, v, K, agg_flow="svc", alpha=alpha, emit_all=True)
    assert res.stats["stage0_path"] == path and allp.stats["stage0_path"] == path
    if alpha not in (0.9, 1.0):
        assert want["n_anomalies"] > (10 if form.startswith("classes") else 1000)


# ------------------------------------------------------------------ B2: the series entry points
def series_cases(golden):
    rng = np.random.default_rng(41)
    cases = [[int(x) for x in golden["throughput_list"]]]
    for n in (1, 7, 300):
        x = (3_000_000_000 + rng.integers(-40_000_000, 40_000_000, size=n)).astype(np.uint64)
        x[::5] *= np.uint64(3)
        cases.append(x.tolist())
    return cases


@pytest.mark.parametrize("alpha", [0.3, 1 / 3])
def test_series_ewma_alpha(engine, golden, alpha):
    for x in series_cases(golden):
        assert engine.series_ewma(x, alpha).tolist() == orc.calculate_ewma(x, alpha), len(x)
        sd = orc.stddev_samp_series(orc.u64_to_f64(x))                       # None for the series of one point: no verdicts
        for s in (sd, None if sd is None else sd / 2, golden["stddev"]):
            assert engine.series_ewma_anomaly(x, s, alpha).tolist() == orc.calculate_ewma_anomaly(x, s, alpha), len(x)
    x = series_cases(golden)[0]
    assert any(orc.calculate_ewma_anomaly(x, golden["stddev"], alpha)) and not all(orc.calculate_ewma_anomaly(x, golden["stddev"], alpha))


# ------------------------------------------------------------------ B3: streaming EWMA
@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("n_rows,K,T,cuts", [(3000, 7, 64, (1, 2, 3, 60)), (60000, 200, 120, (40, 80))])
def test_stream_ewma_alpha(engine, n_rows, K, T, cuts, form):
    """k_stream (dense batches) and k_stream_points (sparse batches) at alpha 0.3: rows and state against the streaming oracle batch
    by batch, the final state against the batch job over all rows"""
    alpha = 0.3
    k, t, v = orc.synth_rows(0, n_rows, K, T)
    bucket = (t - orc.SYNTH_T_BASE) // orc.SYNTH_T_STEP
    edges = (0,) + tuple(cuts) + (T,)
    st = engine.state_create(K)
    ost = so.StreamState(K)
    n_rows_out = 0
    try:
        with engine.plan(sparse="never" if form == "dense" else "always"):
            for lo, hi in zip(edges[:-1], edges[1:]):
                sel = (bucket >= lo) & (bucket < hi)
                got = engine.run_stream(st, k[sel], t[sel], v[sel], agg_flow="svc", alpha=alpha)
                want = so.run_stream(ost, k[sel], t[sel], v[sel], "sum", alpha=alpha)
                assert (got.stats["stage0_path"] in (4, 8)) == (form == "sparse"), got.stats["stage0_path"]
                assert got.n_rows == want["key_id"].size
                for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev"):
                    assert (got[f] == want[f]).all(), (lo, hi, f)
                n_rows_out += got.n_rows
        state = st.export()
    finally:
        st.close()
    assert n_rows_out > K
    for f in ("n", "avg", "m2", "ewma", "last_t"):
        assert (state[f] == getattr(ost, f)).all(), f
    job = orc.run_job("EWMA", k, t, v, agg_flow="svc", alpha=alpha)
    kk, ptr = job["keys"].astype(np.int64), job["ptr"]
    n = state["n"][kk].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        stream_sigma = np.sqrt(state["m2"][kk] / (n - 1.0))
    assert (np.diff(ptr) == state["n"][kk]).all()
    assert (stream_sigma[job["has_sigma"]] == job["sigma"][job["has_sigma"]]).all()
    assert (state["ewma"][kk] == job["calc_all"][ptr[1:] - 1]).all()
    assert (job["calc_all"][ptr[1:] - 1] != orc.run_job("EWMA", k, t, v, agg_flow="svc")["calc_all"][ptr[1:] - 1]).all()


# ------------------------------------------------------------------ B4: the DBSCAN job
@pytest.fixture(scope="module")
def spread_P(P):
    """per operator: (max - min, point count) of every key's series, from the oracle's Stage 0"""
    out = {}
    for agg, op in (("svc", "sum"), ("", "max")):
        pk, pt, pv = orc.stage0(*P, op)
        keys, ptr = orc.series_offsets(pk)
        x = orc.u64_to_f64(pv)
        assert keys.size == K_P
        out[agg] = (np.maximum.reduceat(x, ptr[:-1]) - np.minimum.reduceat(x, ptr[:-1]), np.diff(ptr))
    return out


# (operator, eps, min_samples, keys on the work list, noise points): the oracle's figures for P
DBSCAN_P = [
    ("", 5e5, 4, 9000, 19_963), ("svc", 2.5e6, 4, 9000, 36_131), ("svc", 2.5e6, 9, 9000, 94_831),      # every key listed, mixed verdicts
    ("", 2.5e6, 9, 7909, 206), ("svc", 4e9, 12, 7490, 3451),            # more listed keys than compact_cap(g) = 4096, beside settled ones
    ("svc", 2.0**64, 1, 0, 0), ("", 2.0**64, 1, 0, 0), ("svc", 2.0**64, 4, 0, 0), ("", 2.0**64, 4, 0, 0),      # nothing listed
    ("svc", 2.0**64, 60, 9000, N_POINTS_P), ("", 2.0**64, 60, 9000, N_POINTS_P),        # n < min_samples everywhere: every point noise
    ("svc", 0.5, 2, 9000, None), ("", 0.5, 2, 9000, None),              # an eps that is no integer: only equal values are neighbours
]


@pytest.mark.parametrize("agg,eps,min_samples,n_listed,n_noise", DBSCAN_P,
                         ids=["%s-eps%g-ms%d" % ("sum" if c[0] else "max", c[1], c[2]) for c in DBSCAN_P])
def test_dbscan_job_eps_and_min_samples(engine, stage0, P, spread_P, agg, eps, min_samples, n_listed, n_noise):
    """The tile pass in settle mode (SettleArgs.eps, .min_samples) lists a key when max - min > eps or n < min_samples and settles the
    rest; the list kernels judge the listed keys, from contiguous series up to compact_cap keys and from the grid beyond."""
    spread, n = spread_P[agg]
    listed = (spread > eps) | (n < min_samples)
    assert listed.sum() == n_listed
    if 0 < n_listed < K_P:
        assert 4096 < listed.sum() < K_P          # past compact_cap(g) = min(K, max(K / 8, 4096)) and not the whole table
    k, t, v = P
    res, want = check_job(engine, "DBSCAN", k, t, v, K_P, agg_flow=agg, eps=eps, min_samples=min_samples)
    assert want["n_points"] == N_POINTS_P
    if n_noise is None:
        assert 0.99 * N_POINTS_P < want["n_anomalies"] <= N_POINTS_P
    else:
        assert want["n_anomalies"] == n_noise
    if stage0 != "v1":
        assert res.stats["stage0_path"] in (2, 3)


@pytest.fixture(scope="module")
def overflow_values():
    """the overflow_values table of test_job_dbscan_settled_in_the_tile_pass: 3 in 1000 values beyond the packed records' 2^49"""
    rng = np.random.default_rng(11)
    k, t, v = orc.synth_rows(0, 600_000, 3000, 100)
    v = v.copy()
    sel = rng.random(v.size) < 0.003
    v[sel] = rng.integers(2**50, 2**63, size=int(sel.sum()), dtype=np.uint64)
    return k, t, v


@pytest.mark.parametrize("eps,min_samples", [(2.5e6, 9), (1e5, 4)])
def test_dbscan_job_parameters_with_values_on_the_overflow_list(engine, stage0, overflow_values, eps, min_samples):
    """the overflow_values table of test_job_dbscan_settled_in_the_tile_pass (values beyond the packed records: the whole job takes
    the redo walk).  At eps 2.5e6, min_samples 9 the noise points are those of the defaults, the values beyond 2^50; at eps 1e5,
    min_samples 4 there are thirty times as many, so a redo walk on the default eps would show."""
    k, t, v = overflow_values
    res, want = check_job(engine, "DBSCAN", k, t, v, 3000, agg_flow="", eps=eps, min_samples=min_samples)
    usual = orc.run_job("DBSCAN", k, t, v, agg_flow="")["n_anomalies"]
    assert 1000 < usual < want["n_points"] // 10
    assert want["n_anomalies"] == usual if eps == 2.5e6 else want["n_anomalies"] > 10 * usual
    if stage0 != "v1":
        assert res.stats["stage0_path"] in (2, 3)


@pytest.mark.parametrize("eps,min_samples", [(5e5, 4), (4e9, 12)])
def test_dbscan_job_parameters_on_long_series(engine, few_long_keys, eps, min_samples):
    """series of more than 256 points as a job: k_dbscan_sorted's windows and the wavefront-per-key scan"""
    k, t, v = few_long_keys[70, 1300]
    res, want = check_job(engine, "DBSCAN", k, t, v, 70, agg_flow="svc", eps=eps, min_samples=min_samples)
    assert res.stats["n_buckets"] >= 512 and np.diff(want["ptr"]).max() > 1000
    assert 30 < want["n_anomalies"] < want["n_points"] // 10


@pytest.mark.parametrize("form", list(SPARSE_FORMS))
def test_dbscan_job_parameters_sparse_forms(engine, stage0, day, classes, form):
    """eps 5e5, min_samples 4 on the sparse Stage 0 and on the length classes: more noise than the spikes the defaults find"""
    plan, path = SPARSE_FORMS[form]
    k, t, v, K = classes if form.startswith("classes") else day + (K_DAY,)
    with engine.plan(**plan):
        res, want = check_job(engine, "DBSCAN", k, t, v, K, agg_flow="", eps=5e5, min_samples=4)
        allp = engine.run("DBSCAN", k, t, v, K, agg_flow="", eps=5e5, min_samples=4, emit_all=True)
    assert res.stats["stage0_path"] == path and allp.stats["stage0_path"] == path
    assert want["n_anomalies"] > 1.5 * orc.run_job("DBSCAN", k, t, v, agg_flow="")["n_anomalies"] > 0
