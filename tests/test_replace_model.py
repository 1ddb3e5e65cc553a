"""CPU: the host model of tad_state_replace (tests/replace_model.py) on tables small enough to check by hand, its idempotence, "a ranged
replace of everything is a fresh state fed the batch", and what the seeded scripts of tests/test_gpu_state_replace.py cover."""
import numpy as np
import pytest

import replace_model as rm
from replace_model import ReplaceModel
from state_model import HIST, SER, TIMES, I64, U64

FLAGS = HIST | SER | TIMES


def rows(*pts):
    """(key, time, value) triples -> three columns"""
    a = np.array(pts, dtype=np.int64).reshape(-1, 3)
    return a[:, 0].astype(U64), a[:, 1].astype(I64), a[:, 2].astype(U64)


def table(m):
    return list(zip(m.key.tolist(), m.t.tolist(), m.value.tolist()))


def model(op="sum", K=3):
    m = ReplaceModel(K, FLAGS, op, 0.0)
    m.append(*rows((0, 10, 5), (0, 20, 6), (0, 30, 7), (1, 10, 100), (1, 40, 101), (2, 20, 9)))
    return m


def test_a_point_at_a_held_time_takes_the_new_value_and_is_never_combined():
    for op in ("sum", "max"):
        m = model(op)
        c = m.replace(*rows((0, 20, 1), (1, 40, 2)))
        assert table(m) == [(0, 10, 5), (0, 20, 1), (0, 30, 7), (1, 10, 100), (1, 40, 2), (2, 20, 9)]
        assert [c[f] for f in rm.COUNTERS] == [2, 0, 0, 0, 2, 0, 0]


def test_the_value_op_aggregates_inside_the_batch_only():
    m = model("sum")
    m.replace(*rows((0, 20, 1), (0, 20, 2), (0, 25, 4)))
    assert table(m)[:4] == [(0, 10, 5), (0, 20, 3), (0, 25, 4), (0, 30, 7)]
    m = model("max")
    m.replace(*rows((0, 20, 1), (0, 20, 2)))
    assert table(m)[1] == (0, 20, 2)


def test_the_range_is_half_open_and_erases_on_every_key():
    m = model()
    c = m.replace(*rows((0, 20, 1), (0, 50, 8)), from_t=20, to_t=40, ranged=True)
    # key 0 keeps 10, takes 20, loses 30, gains 50; key 1 keeps 10 and 40 (to_t is exclusive); key 2 loses its only point
    assert table(m) == [(0, 10, 5), (0, 20, 1), (0, 50, 8), (1, 10, 100), (1, 40, 101)]
    assert c["points_replaced"] == 1 and c["points_appended"] == 1 and c["points_inserted"] == 0
    assert c["points_erased"] == 2 and c["keys_emptied"] == 1
    m = model()
    m.replace(*rows(), from_t=10, to_t=11, ranged=True)     # from_t is inclusive
    assert table(m) == [(0, 20, 6), (0, 30, 7), (1, 40, 101), (2, 20, 9)]


def test_bounds_zero_mean_no_bound_and_equal_bounds_mean_nothing():
    m = model()
    assert m.replace(*rows(), from_t=30, ranged=True)["points_erased"] == 2
    assert table(m) == [(0, 10, 5), (0, 20, 6), (1, 10, 100), (2, 20, 9)]
    m = model()
    assert m.replace(*rows(), to_t=20, ranged=True)["points_erased"] == 2
    assert table(m) == [(0, 20, 6), (0, 30, 7), (1, 40, 101), (2, 20, 9)]
    m = model()
    before = table(m)
    c = m.replace(*rows(), from_t=20, to_t=20, ranged=True)
    assert table(m) == before and c["points_erased"] == 0
    c = m.replace(*rows(), from_t=1000, to_t=2000, ranged=True)
    assert table(m) == before and c["points_erased"] == 0
    c = m.replace(*rows((1, 5, 3)), ranged=False)
    assert c["points_inserted"] == 1 and c["points_erased"] == 0 and len(table(m)) == len(before) + 1


def test_keep_from_drops_batch_points_before_they_name_anything():
    m = model()
    c = m.replace(*rows((0, 10, 1), (0, 30, 2)), from_t=0, to_t=0, ranged=True, keep_from=25)
    # (0, 10) is too old: it names nothing, so the old (0, 10) is erased with the rest of R = everything
    assert table(m) == [(0, 30, 2)]
    assert c["points_too_old"] == 1 and c["points_replaced"] == 1 and c["points_erased"] == 5 and c["keys_emptied"] == 2


def test_a_key_emptied_and_refilled_is_not_counted_as_emptied():
    m = model()
    c = m.replace(*rows((2, 99, 4)), from_t=0, to_t=50, ranged=True)
    assert table(m) == [(2, 99, 4)]
    assert c["keys_emptied"] == 2 and c["points_appended"] == 1 and c["points_erased"] == 6


@pytest.mark.parametrize("op", ["sum", "max"])
def test_the_same_call_twice_leaves_the_same_table(op):
    rng = np.random.default_rng(5)
    m = ReplaceModel(40, FLAGS, op, 0.3)
    m.append(rng.integers(0, 40, 600).astype(U64), 1000 + rng.integers(0, 300, 600), rng.integers(1, 1 << 40, 600).astype(U64))
    b = (rng.integers(0, 40, 300).astype(U64), 1100 + rng.integers(0, 300, 300), rng.integers(1, 1 << 40, 300).astype(U64))
    c1 = m.replace(*b, from_t=1150, to_t=1350, ranged=True, keep_from=1120)
    once = table(m)
    snap = m.expected_snapshot()
    c2 = m.replace(*b, from_t=1150, to_t=1350, ranged=True, keep_from=1120)
    assert table(m) == once
    assert c1["points_erased"] > 0 and c1["points_inserted"] > 0 and c1["points_appended"] > 0 and c1["points_replaced"] > 0
    assert c2["points_erased"] == c2["points_inserted"] == c2["points_appended"] == 0
    assert c2["points_replaced"] == c2["batch_points"] - c2["points_too_old"]
    again = m.expected_snapshot()
    for f in ("n", "avg", "m2", "ewma", "last_t"):
        assert np.array_equal(snap["state"][f].view(np.uint64) if snap["state"][f].dtype.itemsize == 8 else snap["state"][f],
                              again["state"][f].view(np.uint64) if again["state"][f].dtype.itemsize == 8 else again["state"][f])


@pytest.mark.parametrize("op", ["sum", "max"])
def test_a_ranged_replace_of_everything_is_a_fresh_model_fed_the_batch(op):
    rng = np.random.default_rng(9)
    m = ReplaceModel(25, FLAGS, op, 0.0)
    m.append(rng.integers(0, 25, 400).astype(U64), 500 + rng.integers(0, 100, 400), rng.integers(1, 1000, 400).astype(U64))
    b = (rng.integers(0, 25, 200).astype(U64), 450 + rng.integers(0, 200, 200), rng.integers(1, 1000, 200).astype(U64))
    m.replace(*b, ranged=True)
    fresh = ReplaceModel(25, FLAGS, op, 0.0)
    fresh.append(*b)
    assert table(m) == table(fresh)
    a, f = m.expected_snapshot(), fresh.expected_snapshot()
    assert np.array_equal(a["series"][1], f["series"][1]) and np.array_equal(a["history"][1], f["history"][1]) and np.array_equal(a["times"], f["times"])


def test_the_scripts_mix_replaces_of_every_kind_with_the_other_calls():
    kinds, variants, flags = set(), set(), set()
    erased = emptied = replaced = 0
    for seed in rm.SEEDS:
        sc = rm.make_script(seed)
        again = rm.make_script(seed)
        assert len(sc["ops"]) == 12 and [o["kind"] for o in sc["ops"]] == [o["kind"] for o in again["ops"]]
        flags.add(sc["flags"])
        n_arima = 0
        for op in sc["ops"]:
            kinds.add(op["kind"])
            n_arima += (op.get("algo") == "ARIMA") + sum(c["algo"] == "ARIMA" for c in op["checks"])
            if op["kind"] == "replace":
                variants.add(op["variant"])
                erased += op["info"]["points_erased"]
                emptied += op["info"]["keys_emptied"]
                replaced += op["info"]["points_replaced"]
        assert n_arima <= 3
    assert {"replace", "append", "merge", "trim", "compact", "resize", "restart"} <= kinds, kinds
    assert len(variants) >= 8, variants
    assert flags == {10, 11}
    assert erased > 100 and replaced > 100 and emptied > 0
