"""GPU: the ARIMA kernels (theia_amd/csrc/tad_arima.hip) at every staging seam and key-chunk edge, against the oracle.

The arithmetic paths of the fit are covered by tests/test_gpu_arima.py; this file sits on both sides of the constants of the INDEXING
around them, where an off-by-one changes results or reads a neighbour's memory:

  kStage = 8           Tpad = roundup8(T); k_arima_prep's batches of eight buckets and their tail loop; the fit's prefetch guard
                       t0 + kStage < p, its last-round count nb = p - t0, the product's renormalisation keyed on (i & 3) == 0
  kArimaChunk = 4096   more than one wavefront per position: blockIdx.x / nchunks -> p, the history and save blocks by blockIdx.x
  64 / 256             k_arima_start's key blocks (blockIdx.x / npos, % npos), k_arima_prep's blocks and its keys_no_result reduction
  arima_carve          tpos takes 4 bytes per cell: an odd K x T must not leave the 64-bit cursors 4-byte aligned
  refill               candidates rejected after the shared cursor handed them out (n_pts[cand] > p, state[cand] == 0); idle lanes read
                       row 0 of ysk, which k_arima_prep never writes when key 0 has no result
  streaming            len8 = roundup8(n) with packed yoff, lo = max(old, 3), the predictions at i < 3 && i >= old made in k_as_prep,
                       k_as_list's union of position ranges, (hcnt[p] + chunk - 1) / chunk wavefronts per position with chunk = 64

Every case compares the engine's rows with orc.run_job — key, time, throughput and stddev equal, algo_calc bit for bit with non-finite
values at the same indices (assert_predictions of tests/job_helpers.py: 1e-6 relative AND bit identity), every verdict, keys_no_result,
arima_fits against the sum of max(n_k - 3, 0) over the keys with a result, kalman_steps against the oracle's counter — for emit_all and
for the anomaly rows.  The streaming cases take the oracle over the concatenated batches, restricted to the batch's points, never the GPU
batch job (which shares arima_fit_body with the code under test).  The tables come from tests/arima_tables.py; tests/test_arima_tables.py
holds them to what they claim on the host.  No case has more than 4097 keys, no grid-T case more than 25 buckets, no other more than 65.

That the cases can fail was checked by seeding faults one at a time into a scratch copy run on the host emulation build of the kernels:
  nb one too large                          every case (the first: test_grid_T_against_the_stage_of_eight[4-70])
  n_pts[cand] >= p for >                    test_grid_T_against_the_stage_of_eight[7-70] (a fit on a rank that has no point: memory fault)
  the refill's row stride g.T for ws.Tpad   the batch cases with T % 8 != 0 and two keys or more (the first: test_grid_T_...[4-70]);
                                            T = 8 and 16 pass, as they must
  (i & 7) == 0 for (i & 3) == 0             every case with a series of 7 points or more (the first: test_grid_T_...[7-70])
  p without the division by nchunks         the 4097-key jobs (the first: the warm-up job of test_key_count_against_64_256_4096[2-17]: memory fault)
  lo = old without the max with 3           test_stream_lengths_packed_back_to_back (a fit at p < 3: memory fault)
  len8 without the rounding                 NO case, and none can: a slot's series is read from yoff[slot] at any alignment (gfx950's global
                                            loads, like x86's, take 16 bytes from an 8-byte aligned address), the values past a series' end
                                            that a staged round picks up are never used, and the slack behind the packed array covers the
                                            last slot's reads — the rounding buys aligned 16-byte loads, not results.  The back-to-back slots
                                            of test_stream_lengths_packed_back_to_back hold everything else about the packed layout."""
import numpy as np
import pytest

import arima_tables as at
from oracle import tad_oracle as orc
from job_helpers import assert_predictions

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("key_id", "flow_end_s", "throughput", "stddev")


def want_rows(w, emit_all, keep=None):
    """the oracle's rows: emit_all — every point of every key with a result (keep: a mask over the points), else its anomalous points"""
    pk, pt, pv = w["points"]
    n = np.diff(w["ptr"])
    sel = np.repeat(np.array([r is not None for r in w["arima_results"]], bool), n)
    if keep is not None:
        sel &= keep
    if not emit_all:
        sel &= w["anomaly_all"]
    return {"key_id": pk[sel], "flow_end_s": pt[sel], "throughput": orc.u64_to_f64(pv)[sel], "stddev": np.repeat(w["sigma"], n)[sel],
            "algo_calc": w["calc_all"][sel], "anomaly": w["anomaly_all"][sel]}


def assert_arima_rows(res, want, emit_all, what):
    assert res.n_rows == want["key_id"].size, (what, res.n_rows, want["key_id"].size)
    for f in ROW_FIELDS:
        assert np.array_equal(np.asarray(res[f]), want[f]), (what, f)
    assert_predictions(res["algo_calc"], want["algo_calc"], what)
    if emit_all:
        assert np.array_equal(np.asarray(res["anomaly"]).astype(bool), want["anomaly"]), (what, "verdicts")      # zero verdict flips


def check_table(engine, tab, dense=True):
    """both row sets and the counters of one table against the oracle; dense: on the table's own lattice (g.T = tab.T)"""
    w = at.want(tab)
    kw = dict(lattice=tab.lattice) if dense else {}
    out = []
    for emit_all in (True, False):
        res = engine.run("ARIMA", tab.key, tab.t, tab.v, tab.K, agg_flow="svc", emit_all=emit_all, **kw)
        what = (tab.name, "emit_all" if emit_all else "anomalies")
        st = res.stats
        if dense:
            assert st["stage0_path"] < 4 and st["n_buckets"] == tab.T, (what, st["stage0_path"], st["n_buckets"])
        assert_arima_rows(res, want_rows(w, emit_all), emit_all, what)
        assert st["n_keys"] == w["n_keys"] and st["n_points"] == w["n_points"], what
        assert st["keys_no_result"] == w["keys_no_result"] == tab.expected_no_result(), what
        assert st["arima_fits"] == tab.expected_fits(), (what, st["arima_fits"], tab.expected_fits())
        assert st["kalman_steps"] == w["kalman_steps"], (what, st["kalman_steps"], w["kalman_steps"])
        if not emit_all:
            assert st["n_anomalies"] == w["n_anomalies"] == res.n_rows
        out.append(res)
    return out


# ---- A. the grid's T against 8 ----
@pytest.mark.parametrize("T,K", at.GRID_CASES)
def test_grid_T_against_the_stage_of_eight(engine, T, K):
    """T = 3: no fit is launched, every key is a key without a result, no rows.  T = 4: one position, one wavefront.  T = 7, 8, 9 and 15,
    16, 17: Tpad = 8 | 8 | 16 and 16 | 16 | 24, the last position's one | one | two staging rounds (nb = 6, 7, 8 and 6, 7, 8 after a
    full round), k_arima_prep with no batch of eight | no tail | a tail of one.  From T = 17 on the job holds every p mod 8; T = 25:
    three rounds, two prefetches.  A fifth of the cells is missing, so a key's p-th point is not at bucket p; every eighth key is whole, so
    the last position has fits.  K = 71 at T = 15, 17, 25: an odd number of cells."""
    tab = at.grid_table(T, K)
    allp, res = check_table(engine, tab)
    if T == 3:
        assert allp.n_rows == res.n_rows == 0 and res.stats["keys_no_result"] == res.stats["n_keys"] == int((tab.lengths > 0).sum()) > 60
        assert res.stats["arima_fits"] == 0


# ---- B. the key count against 64 / 256 / 4096 ----
@pytest.mark.parametrize("K,T", at.KEY_CASES)
def test_key_count_against_64_256_4096(engine, K, T):
    """K = 1: 63 lanes idle for the whole job.  K = 2 with key 0 constant: every idle lane reads row 0 of ysk, which no kernel of this
    job writes — run after a 4097-key job on the same engine, so that the workspace is not fresh.  63 | 64 | 65: k_arima_start's key
    blocks; 255 | 256 | 257: k_arima_prep's blocks; 4095 | 4096 | 4097: one | one | two wavefronts per position, whose position is
    blockIdx.x / nchunks."""
    if K == 2:
        big = at.key_table(4097, 9)
        engine.run("ARIMA", big.key, big.t, big.v, big.K, agg_flow="svc", lattice=big.lattice)
    check_table(engine, at.key_table(K, T))


# ---- C. ragged lengths ----
@pytest.mark.parametrize("K,T,seed,cap", at.RAGGED_CASES)
def test_ragged_lengths(engine, K, T, seed, cap):
    """every series length 0 .. T (cap: 0 .. T - 2, the top positions' wavefronts run dry on their first refill), first buckets that
    vary, holes in every other cycle, keys without a result at ids 0, 63, 64 and K - 1: the refill meets candidates it must reject at
    every position"""
    check_table(engine, at.ragged_table(K, T, seed, cap))


# ---- D. seams inside a series ----
@pytest.mark.parametrize("K,T", at.SEAM_CASES)
def test_seams_inside_a_series(engine, K, T):
    check_table(engine, at.seam_table(K, T))


# ---- E. the rank grid ----
RANK_TABLES = [("ragged",) + at.RAGGED_CASES[0]] + [("seam",) + c for c in at.SEAM_CASES]


@pytest.mark.parametrize("case", RANK_TABLES, ids=["-".join(str(x) for x in c) for c in RANK_TABLES])
def test_rank_grid(engine, case):
    """the sparse Stage 0: T is the longest series and tpos a rank, the same rows"""
    tab = at.ragged_table(*case[1:]) if case[0] == "ragged" else at.seam_table(*case[1:])
    with engine.plan(sparse="always"):
        for res in check_table(engine, tab, dense=False):
            assert res.stats["stage0_path"] == 4, res.stats["stage0_path"]


# ---- F. the streaming list form ----
_STREAM_WANT = {}


def stream_want(case, b):
    if (case.name, b) not in _STREAM_WANT:
        k, t, v = case.concat(b)
        _STREAM_WANT[case.name, b] = orc.run_job("ARIMA", k, t, v, agg_flow="svc")
    return _STREAM_WANT[case.name, b]


def batch_mask(w, batch):
    """the points of the oracle's job that belong to `batch` (one row per point: (key, time) names a point)"""
    pk, pt, _ = w["points"]
    code = lambda k, t: (k.astype(np.uint64) << np.uint64(32)) | (t - at.T0).astype(np.uint64)
    return np.isin(code(pk, pt), code(batch[0], batch[1]))


def check_stream(engine, case):
    """Both batches of a case through run_stream on a fresh state, once per row set; then the whole state through run_state.  Returns
    the state of the emit_all pass (the caller closes it)."""
    keep_state = None
    for emit_all in (False, True):
        st = engine.state_create(case.K, series=True, times=True)
        for b, (bk, bt, bv) in enumerate(case.batches):
            if bk.size == 0:
                continue
            what = (case.name, "batch %d" % b, "emit_all" if emit_all else "anomalies")
            res = engine.run_stream(st, bk, bt, bv, agg_flow="svc", algo="ARIMA", emit_all=emit_all)
            w = stream_want(case, b)
            assert_arima_rows(res, want_rows(w, emit_all, batch_mask(w, (bk, bt))), emit_all, what)
            s = res.stats
            assert s["keys_no_result"] == case.expected_no_result(b), (what, s["keys_no_result"], case.expected_no_result(b))
            assert s["arima_fits"] == case.expected_fits(b), (what, s["arima_fits"], case.expected_fits(b))
            if b == 0:
                assert s["kalman_steps"] == w["kalman_steps"], what        # (a first batch fits every position: the oracle's counter)
        if emit_all:
            keep_state = st
        else:
            st.close()
    return keep_state


def check_run_state(engine, st, case, b, window=(0, 0)):
    """run_state (window (0, 0)) / run_state_window over [from_t, to_t): every point is new, the oracle over the points in the range"""
    k, t, v = case.concat(b)
    m = np.ones(k.size, bool)
    if window[0]:
        m &= t >= window[0]
    if window[1]:
        m &= t < window[1]
    w = orc.run_job("ARIMA", k[m], t[m], v[m], agg_flow="svc") if window != (0, 0) else stream_want(case, b)
    for emit_all in (True, False):
        what = (case.name, window, emit_all)
        if window == (0, 0):
            res = engine.run_state(st, algo="ARIMA", emit_all=emit_all)
        else:
            res = engine.run_state_window(st, window[0], window[1], algo="ARIMA", emit_all=emit_all)
        assert_arima_rows(res, want_rows(w, emit_all), emit_all, what)
        s = res.stats
        n = np.diff(w["ptr"])
        has = np.array([r is not None for r in w["arima_results"]], bool)
        assert s["keys_no_result"] == w["keys_no_result"], what
        assert s["arima_fits"] == int(np.clip(n - 3, 0, None)[has].sum()), what
        assert s["kalman_steps"] == w["kalman_steps"], what
    return w


def test_stream_lengths_packed_back_to_back(engine):
    """n in {7, 8, 9, 15, 16, 17} after the batch, every key touched: slot j + 1's series begins right behind slot j's roundup8(n)"""
    case = at.stream_lengths()
    st = check_stream(engine, case)
    check_run_state(engine, st, case, 1)
    st.close()


def test_stream_old_and_new_around_three(engine):
    """old in {0 .. 4} x 1 .. 4 new points: predictions at p < 3 (k_as_prep), fits from lo = max(old, 3), an untouched key between any
    two touched ones"""
    case = at.stream_old_new()
    st = check_stream(engine, case)
    check_run_state(engine, st, case, 1)
    st.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_stream_touched_keys(engine, m):
    """m touched keys of 600: one lane, a wavefront less one, a full one, one more, a block of k_as_list and one more; slot 0 (m > 1)
    and slot 63 (m > 63) have no result"""
    case = at.stream_touched(m)
    st = check_stream(engine, case)
    if m == 257:
        check_run_state(engine, st, case, 1)
    st.close()


@pytest.mark.parametrize("m", [63, 64, 65])
def test_stream_fits_at_one_position(engine, m):
    """63 | 64 | 65 fits at position 8: one wavefront with an idle lane, a full one, two"""
    case = at.stream_fits_at(8, m)
    assert case.fits_per_position(1)[8] == m
    check_stream(engine, case).close()


def test_state_window_cuts_a_series(engine):
    """run_state_window over ranges that leave 5 | 4 | 3, 6 | 5 | 4, 10 | 9 | 8 and 4 | 5 | 6 points of every series"""
    case = at.window_cut_state()
    st = check_stream(engine, case)
    check_run_state(engine, st, case, 0)
    bucket = lambda b: at.T0 + at.STEP * b
    lens = set()
    for window in ((0, bucket(5)), (0, bucket(6)), (0, bucket(10)), (bucket(8), 0)):
        w = check_run_state(engine, st, case, 0, window)
        lens |= set(np.diff(w["ptr"]).tolist())
    assert {3, 4, 8} <= lens
    st.close()
