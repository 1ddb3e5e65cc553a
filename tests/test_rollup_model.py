"""CPU: the host model of tad_state_rollup (tests/rollup_model.py) alone — the consequences include/tad.h states, checked on the model
before any kernel is asked to have them: idempotence, composition, commuting tiers, the bucketed rows of a rolled table against those of
the raw one (tests/buckets_model.py), negative times and a non-zero origin, the counters; and what the seeded scripts of
tests/test_gpu_rollup_sequences.py cover."""
import numpy as np
import pytest

import buckets_model as B
import rollup_model as R
from rollup_model import HIST, SER, TIMES, I64, U64, RollupModel


def table(seed, K=7, span=20000, t0=1_700_000_000, density=0.3):
    rng = np.random.default_rng(seed)
    ks, ts = [], []
    for k in range(K):
        t = t0 + np.flatnonzero(rng.random(span) < density * (k + 1) / K)
        ks.append(np.full(t.size, k)), ts.append(t)
    k, t = np.concatenate(ks).astype(U64), np.concatenate(ts).astype(I64)
    v = rng.integers(1, 1 << 62, size=k.size).astype(U64) * U64(5)           # sums of a bucket wrap
    return k, t, v


def model(seed, op="sum", **kw):
    m = RollupModel(kw.pop("K", 7), HIST | SER | TIMES, op, 0.3)
    m._set(*table(seed, K=m.num_keys, **kw))
    return m


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.points(), b.points()))


@pytest.mark.parametrize("op", ["sum", "max"])
def test_idempotent_and_the_counters(op):
    m = model(1, op)
    k, t, v = (a.copy() for a in m.points())
    before = 1_700_000_000 + 12345
    s1 = m.rollup(before, 60, 7)
    b = s1["before_t"]
    assert b == 7 + 60 * ((before - 7) // 60) and b <= before < b + 60
    assert s1["points_before"] == k.size and s1["points_rolled"] == int((t < b).sum()) > 0
    assert s1["points_after"] == m.key.size == k.size - s1["points_rolled"] + s1["buckets"] and 0 < s1["buckets"] < s1["points_rolled"]
    assert s1["keys_changed"] == m.num_keys
    assert np.array_equal(m.t[m.t >= b], t[t >= b]) and ((m.t[m.t < b] - 7) % 60 == 0).all()
    bk, bt, bv = B.fold(k[t < b], t[t < b], v[t < b], 60, 7, op)
    assert np.array_equal(m.key[m.t < b], bk) and np.array_equal(m.t[m.t < b], bt) and np.array_equal(m.value[m.t < b], bv)
    once = tuple(a.copy() for a in m.points())
    s2 = m.rollup(before, 60, 7)
    assert all(np.array_equal(x, y) for x, y in zip(once, m.points()))
    assert s2["points_rolled"] == s2["buckets"] == s1["buckets"] and s2["keys_changed"] == 0 and s2["points_after"] == s2["points_before"]


@pytest.mark.parametrize("op", ["sum", "max"])
def test_composition_60_then_3600_is_3600(op):
    a, b = model(2, op), model(2, op)
    before = (1_700_000_000 + 15000) // 3600 * 3600              # "the same bound": a bucket start of the coarser call, so both floor to it
    assert a.rollup(before + 59, 60, 0)["before_t"] == before
    assert a.rollup(before, 3600, 0)["before_t"] == before
    b.rollup(before, 3600, 0)
    assert same(a, b)
    # a congruent origin composes too; an origin that is not congruent does not
    c, d, e = model(2, op), model(2, op), model(2, op)
    before = before + 1000
    c.rollup(before, 60, 40), c.rollup(before, 3600, 1000)
    assert d.rollup(before, 3600, 1000)["before_t"] == before
    assert 1000 % 60 == 40 and same(c, d)
    e.rollup(before, 60, 0), e.rollup(before, 3600, 1000)
    if op == "sum":                                             # (a maximum may not notice the seconds that changed bucket)
        assert not same(e, d)


def test_tiers_commute():
    t0 = 1_700_000_000
    a, b = model(3), model(3)
    old, recent = t0 + 7200, t0 + 15000
    a.rollup(old, 3600, 0), a.rollup(recent, 60, 0)
    b.rollup(recent, 60, 0), b.rollup(old, 3600, 0)
    assert same(a, b)
    b_old, b_recent = old // 3600 * 3600, recent // 60 * 60
    assert (a.t < b_old).any() and ((a.t[a.t < b_old] % 3600) == 0).all()
    mid = a.t[(a.t >= b_old) & (a.t < b_recent)]
    assert (mid % 60 == 0).all() and (mid % 3600 != 0).any() and (a.t[a.t >= b_recent] % 60 != 0).any()


@pytest.mark.parametrize("op", ["sum", "max"])
def test_bucketed_rows_of_the_rolled_table_equal_the_raw_tables(op):
    raw, rolled = model(4, op), model(4, op)
    before = 1_700_000_000 + 13000
    st = rolled.rollup(before, 60, 20)
    assert st["points_after"] < st["points_before"]
    for mult, origin in ((1, 20), (5, 20), (5, 260), (60, 20)):
        assert origin % 60 == 20
        want = B.fold(*raw.points(), 60 * mult, origin, op)
        got = B.fold(*rolled.points(), 60 * mult, origin, op)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), (mult, origin)
        # a window whose bounds are bucket starts of the call
        lo, hi = (int(B.bucket_start(1_700_000_000 + x, 60 * mult, origin)) for x in (4000, 16000))
        wr, wl = (raw.t >= lo) & (raw.t < hi), (rolled.t >= lo) & (rolled.t < hi)
        want = B.fold(raw.key[wr], raw.t[wr], raw.value[wr], 60 * mult, origin, op)
        got = B.fold(rolled.key[wl], rolled.t[wl], rolled.value[wl], 60 * mult, origin, op)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), ("window", mult, origin)
    # not a multiple: differs
    assert not np.array_equal(B.fold(*raw.points(), 90, 0, op)[2], B.fold(*rolled.points(), 90, 0, op)[2])


def test_negative_times_and_the_bound_itself():
    m = model(5, t0=-9000, span=12000)
    k, t, v = (a.copy() for a in m.points())
    assert (t < 0).any() and (t > 0).any()
    st = m.rollup(-100, 600, 250)
    b = st["before_t"]
    assert b == -350 and (b - 250) % 600 == 0                   # floor, not truncation: -100 lies in [-350, 250)
    assert np.array_equal(m.t[m.t >= b], t[t >= b])
    starts = m.t[m.t < b]
    assert ((starts - 250) % 600 == 0).all() and starts.min() < -8400
    # a point exactly at the bound stays, the one a second below it moves
    one = RollupModel(1, SER | TIMES, "sum", 0.0)
    one._set(np.zeros(3, U64), np.array([b - 1, b, b + 1], I64), np.array([1, 2, 4], U64))
    one.rollup(b, 600, 250)
    assert one.t.tolist() == [b - 600, b, b + 1] and one.value.tolist() == [1, 2, 4]
    one.rollup(b + 599, 600, 250)                               # floored to b again
    assert one.t.tolist() == [b - 600, b, b + 1]
    one.rollup(b + 600, 600, 250)
    assert one.t.tolist() == [b - 600, b] and one.value.tolist() == [1, 6]


def test_moments_of_the_snapshot_follow_the_folded_series():
    m = model(6, K=3, span=500)
    m.rollup(1_700_000_000 + 400, 50, 0)
    snap = m.expected_snapshot()
    n, last = m.per_key()
    assert np.array_equal(snap["state"]["n"], n) and np.array_equal(snap["state"]["last_t"], last)
    assert np.array_equal(snap["series"][1], m.value) and np.array_equal(snap["times"], m.t)
    assert np.array_equal(np.sort(snap["history"][1][:n[0]]), snap["history"][1][:n[0]])


@pytest.mark.parametrize("seed", R.SEEDS)
def test_the_scripts(seed):
    sc = R.make_script(seed)
    assert sc == sc | {"ops": sc["ops"]} and R.make_script(seed)["ops"][-1]["kind"] == sc["ops"][-1]["kind"]      # a function of the seed
    kinds = [op["kind"] for op in sc["ops"]]
    assert kinds.count("rollup") >= 2 and len(kinds) == R.sm.N_OPS


def test_what_the_seed_set_covers():
    ops = [op for seed in R.SEEDS for op in R.make_script(seed)["ops"]]
    roll = [op for op in ops if op["kind"] == "rollup"]
    assert {op["variant"] for op in roll} >= {"old", "most", "all", "again", "coarser"}
    assert sum(op["info"]["points_after"] < op["info"]["points_before"] for op in roll) >= 8
    assert any(op["info"]["points_rolled"] and op["info"]["keys_changed"] == 0 for op in roll)           # rewritten, nothing folded
    assert any(op["origin"] for op in roll)
    for a, b in zip(ops, ops[1:]):                                                                      # each of these follows a roll-up somewhere
        if a["kind"] == "rollup":
            a.setdefault("next", b["kind"])
    assert {op.get("next") for op in roll} >= {"append", "merge", "trim", "compact", "restart", "rollup"}
    assert {sc["flags"] & HIST for sc in map(R.make_script, R.SEEDS)} == {0, HIST}
    assert {R.make_script(s)["op"] for s in R.SEEDS} == {"sum", "max"}
