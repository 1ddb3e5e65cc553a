"""Host checks of tests/arima_tables.py: every table tests/test_gpu_arima_boundaries.py runs is what its builder claims, judged by the
oracle alone (orc.run_job("ARIMA", ...)), so that a green GPU comparison means something.

* keys_no_result equals the number of keys built with <= 3 points, constant, or holding a zero: exact counts.
* at most 1 % of the predictions are NaN (a fit whose optimiser walked into a non-finite likelihood).  A condition on the INPUTS: the
  GPU comparison leaves no point out (NaN is compared index by index), but a table that is mostly NaN would test little.  A table
  over the cap gets another seed, not a looser cap.  Measured: ragged(131, 41) 0.24 %, ragged(259, 65) 0.06 %, ragged(4097, 17) 0.67 %,
  synth_rows 4097 x 9 0.33 %, 4097 x 17 0.14 %; no batch table above 0.67 %, no stream table above 0.95 %.
  Infinite predictions are another matter and are printed beside the NaN share: a short series (4 to 9 points) whose Box-Cox lambda
  is so negative that x ** lambda underflows has y = -1 / lambda at every point, and inv_boxcox returns +inf for all of them, the
  first three included — the reference's own arithmetic, compared value by value on the GPU side like any other.  Their share is a
  property of the series lengths a table must have (5 % of the points of 4097 keys x 9 buckets, a fifth of the 29 four-point keys
  of the T = 4 grid), not of a seed.  What is asserted instead: at every position that has fits, finite fitted predictions
  exist — no position of the fit is checked on non-finite values alone.
* n_anomalies > 0: the anomaly rows of the GPU comparison are not an empty set.
* the per-position fit counts computed on the host have the stated values: 0 at the capped positions, 63 / 64 / 65 at p* for the
  stream tables.
* each table's oracle time is printed (pytest -s): measured 0.01 to 0.7 s a table, the 4097-key ones included."""
import numpy as np
import pytest

import arima_tables as at
from oracle import tad_oracle as orc

TABLES = list(at.all_tables())


def shares(w):
    """(NaN share, infinite share) of the predictions of the keys with a result; finite fitted predictions per position"""
    n = np.diff(w["ptr"])
    sel = np.repeat(np.array([r is not None for r in w["arima_results"]], bool), n)
    calc = w["calc_all"][sel]
    rank = (np.arange(w["calc_all"].size) - np.repeat(w["ptr"][:-1], n))[sel]
    finite_at = np.bincount(rank[np.isfinite(calc)], minlength=int(n.max()) if n.size else 0)
    if calc.size == 0:
        return 0.0, 0.0, finite_at
    return float(np.isnan(calc).mean()), float(np.isinf(calc).mean()), finite_at


def describe(name, K, T, fits, w):
    nan, inf, finite_at = shares(w)
    print("%-50s K %5d T %3d points %6d fits %6d no-result %4d NaN %.2f %% inf %.2f %% anomalies %5d oracle %.2f s"
          % (name, K, T, w["n_points"], fits, w["keys_no_result"], 100 * nan, 100 * inf, w["n_anomalies"], w.get("seconds", 0.0)))
    return nan, finite_at


@pytest.mark.parametrize("tab", TABLES, ids=[t.name for t in TABLES])
def test_table_is_what_it_claims(tab):
    w = at.want(tab)
    nan, finite_at = describe(tab.name, tab.K, tab.T, tab.expected_fits(), w)
    # the lattice: one row per point, the builder's lengths, nothing outside [0, T)
    b = (tab.t - at.T0) // at.STEP
    assert ((tab.t - at.T0) % at.STEP == 0).all() and b.min() >= 0 and b.max() < tab.T
    assert w["n_points"] == tab.key.size or tab.name.startswith("synth")
    assert w["n_keys"] == int((tab.lengths > 0).sum())
    assert np.array_equal(np.diff(w["ptr"]), tab.lengths[w["keys"].astype(np.int64)])
    # keys without a result: exact, and exactly the ones built that way
    assert w["keys_no_result"] == tab.expected_no_result()
    has = np.zeros(tab.K, bool)
    has[w["keys"].astype(np.int64)] = [r is not None for r in w["arima_results"]]
    assert np.array_equal(has, tab.with_result())
    assert tab.expected_fits() == int(tab.fits_per_position().sum())
    assert nan <= at.NAN_CAP, nan
    cnt = tab.fits_per_position()
    assert (finite_at[3:][cnt[3:finite_at.size] > 0] > 0).all(), (cnt.tolist(), finite_at.tolist())
    if tab.T > 3:
        assert w["n_anomalies"] > 0
    else:
        assert w["n_anomalies"] == 0 and not has.any() and w["keys_no_result"] == w["n_keys"] > 0


@pytest.mark.parametrize("T,K", at.GRID_CASES)
def test_grid_tables(T, K):
    tab = at.grid_table(T, K)
    full = K * T
    assert 0.7 * full <= tab.lengths.sum() <= 0.9 * full            # a fifth of the cells removed
    assert (tab.lengths[::8] == T).all() and (tab.lengths < T).sum() > K // 3
    if T >= 4:
        cnt = tab.fits_per_position()
        assert (cnt[3:] >= 9).all() and (T < 7 or cnt[3] > cnt[-1])          # every position 3 .. T - 1 has fits: from T = 17 on every p mod 8
    if K % 2:
        assert (K * T) % 2 == 1                                     # the odd-cell carve: tpos ends on an odd multiple of 4 bytes


@pytest.mark.parametrize("K,T", at.KEY_CASES)
def test_key_tables(K, T):
    tab = at.key_table(K, T)
    assert tab.lengths.size == K and (tab.lengths[-1] > 3 or K == 2)
    if K == 2:
        assert tab.no_result == (0,) and tab.lengths[0] == T and tab.lengths[1] > 3     # key 0, the row idle lanes read, is never written
    if K >= 4095:
        assert (tab.lengths > 3).mean() > 0.95


@pytest.mark.parametrize("K,T,seed,cap", at.RAGGED_CASES)
def test_ragged_tables(K, T, seed, cap):
    plain = at.ragged(K, T, seed, cap)
    top = T if cap is None else cap
    assert np.array_equal(plain.lengths, np.arange(K) % (top + 1))
    assert set(plain.lengths.tolist()) == set(range(top + 1))            # every series length occurs
    s = at.series_of(plain)
    firsts = {int(b[0]) for b, _ in s.values()}
    assert len(firsts) >= min(T // 2, 8)                                 # the first bucket varies
    assert min(int(b[0]) for b, _ in s.values()) == 0 and max(int(b[-1]) for b, _ in s.values()) == T - 1
    for k, (b, _) in s.items():
        holes = int(b[-1] - b[0] + 1 - b.size)
        cycle = k // (top + 1)
        if cycle % 2 == 0:
            assert holes == 0, k
    holed = [k for k, (b, _) in s.items() if b[-1] - b[0] + 1 > b.size]
    assert len(holed) >= (K // (top + 1) // 2) * (top // 2)              # the odd cycles have holes
    tab = at.ragged_table(K, T, seed, cap)
    assert tab.no_result == tuple(at.lane_edges(K)) and {0, 63, 64, K - 1} <= set(tab.no_result)
    cnt = tab.fits_per_position()
    if cap is not None:
        assert (cnt[cap:] == 0).all() and cnt[cap - 1] > 0                # the top positions have no fit at all
    else:
        assert (cnt[3:] > 0).all()
    if K > 4096:
        assert cnt[3] > 64                                                # more than one refill round per wavefront


@pytest.mark.parametrize("K,T", at.SEAM_CASES)
def test_seam_tables(K, T):
    tab = at.seam_table(K, T)
    s = at.series_of(tab)
    assert (K * T) % 2 == T % 2
    for k, (b, _) in s.items():
        c = k % at.SEAM_CLASSES
        if c == 1:
            assert b.tolist() == [5, 6, 7, 8, 9, 10]
        if c == 2 and T % 8:
            assert b[0] >= T - T % 8 and b.size == T % 8
        if c == 3:
            assert not set(b.tolist()) & {7, 8, 15, 16} and b.size == T - sum(h < T for h in (7, 8, 15, 16))
        if c == 7:
            assert b.tolist() == list(range(8))
    assert tab.expected_no_result() == (sum(1 for k in range(K) if k % at.SEAM_CLASSES == 2) if T == 17 else 0)


# ---- the stream tables ----
STREAM = [at.stream_lengths(), at.stream_old_new(), at.window_cut_state()] + [at.stream_fits_at(8, m) for m in (63, 64, 65)] + \
         [at.stream_touched(m) for m in (1, 63, 64, 65, 257)]


@pytest.mark.parametrize("case", STREAM, ids=[c.name for c in STREAM])
def test_stream_case_is_what_it_claims(case):
    for b in (0, 1):
        if case.batches[b][0].size == 0:
            continue
        k, t, v = case.concat(b)
        w = orc.run_job("ARIMA", k, t, v, agg_flow="svc")
        n = case.old + (case.new if b else 0)
        assert np.array_equal(np.diff(w["ptr"]), n[w["keys"].astype(np.int64)]) and w["n_keys"] == int((n > 0).sum())
        has = np.zeros(case.K, bool)
        has[w["keys"].astype(np.int64)] = [r is not None for r in w["arima_results"]]
        assert np.array_equal(has, case.with_result(b)), (case.name, b)
        nan, finite_at = describe("%s batch %d" % (case.name, b), case.K, int(n.max()), case.expected_fits(b), w)
        assert nan <= at.NAN_CAP, nan
        assert w["n_anomalies"] > 0
        print("    touched %3d of %3d keys, fits per position %s" % (case.touched(b).size, case.K, case.fits_per_position(b).tolist()))


@pytest.mark.parametrize("m", [63, 64, 65])
def test_stream_fits_at_one_position(m):
    case = at.stream_fits_at(8, m)
    cnt = case.fits_per_position(1)
    assert cnt[8] == m and (cnt[[7, 9]] > 65).all()          # one wavefront up to 64 fits, two from 65 on; its neighbours take two anyway
    assert 0 < case.touched().size < case.K


def test_stream_shapes():
    c = at.stream_lengths()
    n = c.old + c.new
    assert set(n.tolist()) == {7, 8, 9, 15, 16, 17} and (c.new > 0).all()          # every key touched: the slots are back to back
    assert {(int(a), int(b)) for a, b in zip(n[:-1], n[1:])} >= {(7, 8), (8, 9), (9, 15), (15, 16), (16, 17), (17, 7)}
    c = at.stream_old_new()
    t = c.touched()
    assert {(int(c.old[k]), int(c.new[k])) for k in t} == {(o, w) for o in range(5) for w in range(1, 5)}
    assert (np.diff(t) == 2).all()                                                  # an untouched key between any two touched ones
    for m in (1, 63, 64, 65, 257):
        c = at.stream_touched(m)
        t = c.touched()
        assert t.size == m and c.K == 600 and (np.diff(t) >= 2).all()
        assert c.bad == tuple(int(t[i]) for i in (0, 63) if i < m and m > 1)        # slot 0 and slot 63 have no result
        assert not c.with_result()[list(c.bad)].any()
    c = at.window_cut_state()
    assert (c.old == 12).all() and set(c.first.tolist()) == {0, 1, 2}
