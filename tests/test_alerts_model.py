"""Host: the change report's model (tests/alerts_model.py) checked on hand-made tables, and the rules the header promises restated on the
merge and replace models: what does not change a key, idempotent re-reads, keys_changed <= keys_touched."""
import numpy as np

import alerts_model as am
import replace_model as rm
import state_model as sm
from alerts_model import NO_CHANGE, diff_points, table

SER_TIMES = sm.SER | sm.TIMES
T0 = 1_700_000_000


def test_diff_of_equal_tables_reports_nothing():
    w = table(([0, 0, 2], [T0, T0 + 1, T0], [5, 6, 7]))
    d = diff_points(w, w, 4)
    assert d["key_since"].tolist() == [NO_CHANGE] * 4
    assert (d["keys_changed"], d["points_changed"], d["min_t"], d["max_t"]) == (0, 0, 0, 0)


def test_diff_finds_added_removed_and_revalued_points():
    w0 = table(([0, 0, 0, 1, 2, 2], [T0, T0 + 2, T0 + 4, T0 + 1, T0 + 3, T0 + 9], [1, 2, 3, 4, 5, 6]))
    # key 0: T0 + 2 revalued, T0 + 3 added; key 1: its only point removed; key 2: untouched; key 3: a first point
    w1 = table(([0, 0, 0, 0, 2, 2, 3], [T0, T0 + 2, T0 + 3, T0 + 4, T0 + 3, T0 + 9, T0 + 7], [1, 9, 8, 3, 5, 6, 1]))
    d = diff_points(w0, w1, 5)
    assert d["key_since"].tolist() == [T0 + 2, T0 + 1, NO_CHANGE, T0 + 7, NO_CHANGE]
    assert (d["keys_changed"], d["points_changed"], d["min_t"], d["max_t"]) == (3, 4, T0 + 1, T0 + 7)


def test_diff_takes_the_smallest_time_whatever_the_order_of_the_rows():
    w0 = table(([1, 1, 1], [T0 + 5, T0 + 1, T0 + 3], [1, 1, 1]))
    w1 = table(([1, 1, 1], [T0 + 3, T0 + 5, T0 + 1], [2, 2, 1]))
    d = diff_points(w0, w1, 2)
    assert d["key_since"].tolist() == [NO_CHANGE, T0 + 3] and d["points_changed"] == 2 and d["max_t"] == T0 + 5


def loaded(op):
    m = am.AlertsModel(4, SER_TIMES, op, 0.0)
    m.append(*table(([0, 0, 0, 1, 1, 3], [T0, T0 + 2, T0 + 4, T0, T0 + 2, T0 + 6], [10, 20, 30, 40, 50, 60])))
    return m


def test_sum_merge_of_zero_and_max_merge_of_no_more_change_nothing():
    m = loaded("sum")
    c = m.merge(*table(([0, 1], [T0 + 2, T0], [0, 0])))
    assert c["points_combined"] == 2 and c["changes"]["keys_changed"] == 0 and c["changes"]["points_changed"] == 0
    c = m.merge(*table(([0, 1], [T0 + 2, T0], [0, 7])))
    assert c["changes"]["key_since"].tolist() == [NO_CHANGE, T0, NO_CHANGE, NO_CHANGE] and c["changes"]["points_changed"] == 1
    m = loaded("max")
    c = m.merge(*table(([0, 0, 1], [T0 + 2, T0 + 4, T0], [20, 29, 1])))
    assert c["points_combined"] == 3 and c["changes"]["keys_changed"] == 0
    c = m.merge(*table(([0, 0, 1], [T0 + 2, T0 + 4, T0], [20, 31, 1])))
    assert c["changes"]["key_since"].tolist() == [T0 + 4, NO_CHANGE, NO_CHANGE, NO_CHANGE]


def test_replace_by_the_held_value_changes_nothing_and_a_reread_is_idempotent():
    m = loaded("sum")
    held = table(([0, 1], [T0 + 4, T0 + 2], [30, 50]))
    assert m.replace(*held)["changes"]["keys_changed"] == 0
    # a ranged re-read: key 0 loses T0 + 2, takes another value at T0 + 4 and gains T0 + 5; key 1 is erased from T0 + 2 on; key 3 too
    batch = table(([0, 0], [T0 + 4, T0 + 5], [31, 1]))
    c = m.replace(*batch, from_t=T0 + 1, to_t=0, ranged=True)
    assert c["changes"]["key_since"].tolist() == [T0 + 2, T0 + 2, NO_CHANGE, T0 + 6]
    assert (c["changes"]["points_changed"], c["changes"]["min_t"], c["changes"]["max_t"]) == (5, T0 + 2, T0 + 6)
    again = m.replace(*batch, from_t=T0 + 1, to_t=0, ranged=True)["changes"]
    assert again["keys_changed"] == 0 and again["points_changed"] == 0 and (again["min_t"], again["max_t"]) == (0, 0)


def test_too_old_points_and_empty_batches_change_nothing():
    m = loaded("sum")
    c = m.merge(*table(([0, 2], [T0 + 1, T0 + 1], [5, 5])), keep_from=T0 + 2)
    assert c["points_too_old"] == 2 and c["changes"]["keys_changed"] == 0
    assert m.merge(*sm._empty())["changes"]["keys_changed"] == 0
    assert m.replace(*sm._empty())["changes"]["keys_changed"] == 0


def test_scripts_changed_keys_are_touched_keys_and_a_repeated_replace_reports_nothing():
    """every merge and replace of the eight seeded scripts: the changed keys are among the keys the call touches (a key of a batch point
    that is kept, or a key with a point inside the range), and the same replace again changes nothing"""
    seen = 0
    for seed in rm.SEEDS:
        script = rm.make_script(seed)
        model = rm.ReplaceModel(script["num_keys"], script["flags"], script["op"], script["alpha"])
        for op in script["ops"]:
            if op["kind"] not in ("merge", "replace"):
                rm.apply(model, op, rows=False)
                continue
            wk, wt, _ = (a.copy() for a in model.points())
            _, d = am.apply_with_changes(model, op)
            keep_from = op.get("keep_from", 0)
            touched = np.zeros(model.num_keys, bool)
            kept = op["t"] >= keep_from if keep_from else np.ones(op["t"].size, bool)
            touched[op["k"][kept].astype(np.int64)] = True
            if op["kind"] == "replace":
                touched[wk[rm.in_range(wt, op["from_t"], op["to_t"], op["ranged"])].astype(np.int64)] = True
            assert not (d["key_since"] != NO_CHANGE)[~touched].any(), (seed, op["kind"])
            assert d["keys_changed"] <= int(touched.sum())
            if op["kind"] == "replace":
                _, again = am.apply_with_changes(model, op)
                assert again["keys_changed"] == 0 and again["points_changed"] == 0, (seed, op.get("variant"))
            seen += 1
    assert seen >= 16
