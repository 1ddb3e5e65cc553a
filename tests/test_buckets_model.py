"""The numpy model of tad_run_state_buckets' view (tests/buckets_model.py) against the oracle's Stage 0 over the floored rows: the model
folds runs of rows already in (key, time) order — what the kernels do —, oracle.tad_oracle.stage0 groups by sorting — what tad_run does —,
and the contract says the two give the same points.  Both operations, times below zero, origins other than 0, sums that wrap mod 2^64 and
maxima >= 2^63; then the since rule against its definition written out point by point.  No GPU, no library."""
import numpy as np
import pytest

import buckets_model as M
from oracle import tad_oracle as orc

U64, I64 = np.uint64, np.int64


def table(seed, K, n, t_lo, t_hi, wide):
    """one row per (key, second) in (key, time) order: what a state holds"""
    rng = np.random.default_rng(seed)
    ks, ts = [], []
    for key in range(K):
        m = int(rng.integers(0, n + 1)) if key % 5 else n
        ks.append(np.full(m, key, U64))
        ts.append(np.sort(rng.choice(np.arange(t_lo, t_hi, dtype=I64), size=m, replace=False)))
    k, t = np.concatenate(ks), np.concatenate(ts)
    if wide:                                                             # 50 .. 63 significant bits, a third with bit 63 set
        v = rng.integers(1 << 49, 1 << 62, size=k.size).astype(U64) | np.where(rng.random(k.size) < 0.33, U64(1 << 63), U64(0))
    else:
        v = rng.integers(1, 4_000_000_000, size=k.size).astype(U64)
    return k, t, v


CASES = [(60, 0), (60, 1), (60, 59), (3600, 0), (3600, 1800), (1, 0), (7, 3), (1 << 20, 12345)]


@pytest.mark.parametrize("op", ["sum", "max"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_the_fold_of_runs_is_stage0_over_the_floored_rows(op, wide):
    k, t, v = table(7 + wide, 23, 400, -5000, 9000, wide)
    assert (t < 0).any() and (t == t.min()).sum() >= 1
    for bucket_s, origin in CASES:
        bk, bt, bv = M.fold(k, t, v, bucket_s, origin, op)
        pk, pt, pv = orc.stage0(k, M.bucket_start(t, bucket_s, origin), v, op)
        assert np.array_equal(bk, pk) and np.array_equal(bt, pt) and np.array_equal(bv, pv), (bucket_s, origin)
        # the floor, against Python's // on the same numbers
        for i in range(0, t.size, 97):
            assert int(M.bucket_start(t[i], bucket_s, origin)) == origin + bucket_s * ((int(t[i]) - origin) // bucket_s)
        assert ((bt - origin) % bucket_s == 0).all() and ((t >= 0) | (M.bucket_start(t, bucket_s, origin) <= t)).all()
        first, lens = M.run_lengths(k, t, bucket_s, origin)
        assert lens.sum() == k.size and first.size == bk.size
        if bucket_s == 1:
            assert bk.size == k.size and np.array_equal(bv, v)
    if wide:
        bk, bt, bv = M.fold(k, t, v, 3600, 0, op)
        first, lens = M.run_lengths(k, t, 3600, 0)
        exact = [sum(int(x) for x in v[f:f + n]) if op == "sum" else max(int(x) for x in v[f:f + n]) for f, n in zip(first, lens)]
        assert [int(x) for x in bv] == [x % (1 << 64) for x in exact]
        if op == "sum":
            assert sum(x >> 64 for x in exact) > 0                      # sums that wrapped
        else:
            assert any(x >= 1 << 63 for x in exact) and any(x < 1 << 63 for x in exact)


def test_times_below_zero_round_down():
    t = np.array([-121, -120, -61, -60, -59, -1, 0, 1, 59, 60], I64)
    assert M.bucket_start(t, 60).tolist() == [-180, -120, -120, -60, -60, -60, 0, 0, 0, 60]
    assert M.bucket_start(t, 60, 59).tolist() == [-121, -121, -61, -61, -61, -1, -1, -1, 59, 59]
    k = np.zeros(t.size, U64)
    bk, bt, bv = M.fold(k, t, np.arange(1, t.size + 1, dtype=U64), 60)
    assert bt.tolist() == [-180, -120, -60, 0, 60] and bv.tolist() == [1, 5, 15, 24, 10]


def test_the_since_rule():
    k, t, v = table(3, 12, 200, 1000, 4000, False)
    K = 12
    for bucket_s, origin in ((60, 0), (60, 17), (600, 0)):
        bk, bt, bv = M.fold(k, t, v, bucket_s, origin)
        ks = np.full(K, M.NO_CHANGE, I64)
        ks[[0, 2, 3, 7, 9]] = [1500, 999, 2017, 5000, 2400]
        for since_t in (0, 2000, 2031):
            got = M.reported(bk, bt, bucket_s, origin, since_t, ks)
            want = np.zeros(bk.size, bool)
            for i in range(bk.size):
                key = int(bk[i])
                if ks[key] == M.NO_CHANGE:
                    continue
                thr = max(int(ks[key]), since_t) if since_t else int(ks[key])
                want[i] = int(bt[i]) >= origin + bucket_s * ((thr - origin) // bucket_s)
            assert np.array_equal(got, want), (bucket_s, origin, since_t)
            # every bucket holding a point at or after the threshold is reported, whole — and no bucket that holds none is
            pb = M.bucket_start(t, bucket_s, origin)
            for key in (0, 2, 3, 9):
                thr = max(int(ks[key]), since_t) if since_t else int(ks[key])
                holds = np.unique(pb[(k == key) & (t >= thr)])
                rep = bt[got & (bk == key)]
                assert np.array_equal(rep, holds) or (rep.size == holds.size + 1 and np.array_equal(rep[1:], holds)), (key, since_t)
        none = M.reported(bk, bt, bucket_s, origin, 0, None)
        assert none.all()
        only_t = M.reported(bk, bt, bucket_s, origin, 2031, None)
        assert np.array_equal(only_t, bt >= M.bucket_start(2031, bucket_s, origin)) and 0 < only_t.sum() < bk.size
