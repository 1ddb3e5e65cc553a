"""The host model of the two dictionaries (tests/dict_model.py) checked on the host: against a second formulation of what the
dictionaries hold, for determinism, and for what its seed set covers.  tests/test_gpu_dict_sequences.py runs the same scripts on a
device; a gap in the scripts is a gap there, so the coverage conditions below are asserted, not measured."""
import collections

import numpy as np
import pytest

import dict_model as dm

SKIP = int(dm.KEY_SKIP)


@pytest.fixture(scope="module")
def scripts():
    return [dm.make_script(seed) for seed in dm.SEEDS]


def ops_of(scripts, kind=None, cls=None, checks=False):
    """(script, index, operation) of every operation — with checks=True the read-only checks behind each count as operations too"""
    out = []
    for sc in scripts:
        if cls is not None and sc["class"] != cls:
            continue
        for i, op in enumerate(sc["ops"]):
            out += [(sc, i, o) for o in [op] + (op["checks"] if checks else []) if kind is None or o["kind"] == kind]
    return out


# ---- 1. the model against a second formulation: every row ever fed, as strings, replayed from scratch ----
class Log:
    """The model numbers codes and ids as it goes and pushes them through remaps.  This side knows no code, no id and no remap: it keeps
    every string and every raw row (the tuple with its strings, not their codes) ever fed, in order, and what a compaction or a
    retirement dropped as a filter at its place in the log; what the dictionaries hold is the log replayed through plain dicts."""

    def __init__(self, sc):
        self.sc, self.events = sc, []

    def replay(self):
        keys, vocabs = {}, [{} for _ in range(1 + max(self.sc["str_cols"].values()))]
        for ev in self.events:
            if ev[0] == "strings":
                for s in ev[2]:
                    vocabs[ev[1]].setdefault(s)
            elif ev[0] == "rows":
                for k in ev[1]:
                    keys.setdefault(k)
            elif ev[0] == "drop_keys":
                for k in ev[1]:
                    del keys[k]
            else:
                vocabs[ev[1]] = {s: None for s in vocabs[ev[1]] if s in ev[2]}
        return list(keys), [list(v) for v in vocabs]

    def feed(self, op):
        sc, kind = self.sc, op["kind"]
        if kind == "encode":
            eff = {}
            for c in sorted(sc["str_cols"]):
                for s in range(op["sides"]):
                    strings, nulls = op["strs"][s][c]
                    eff[(c, s)] = [b"" if nulls is not None and nulls[r] else x for r, x in enumerate(strings)]
                    self.events.append(("strings", sc["str_cols"][c], eff[(c, s)]))
            rows = []
            for s, keep in enumerate((op["keep_a"], op["keep_b"])[:op["sides"]]):
                for r in range(op["n"]):
                    if keep is None or keep[r]:
                        rows.append((s, tuple(eff[(c, s)][r] if c in sc["str_cols"] else int(op["ints"][s][c][r]) for c in range(sc["n_cols"]))))
            self.events.append(("rows", rows))
        elif kind == "compact_keys":
            keys, _ = self.replay()
            self.events.append(("drop_keys", [k for k, r in zip(keys, op["remap"].tolist()) if r == SKIP]))
        elif kind == "retire_strings":
            keys, vocabs = self.replay()
            for v, values in enumerate(vocabs):
                used = {t[c] for _, t in keys for c in sc["str_cols"] if sc["str_cols"][c] == v} | {values[e] for e in op["extras"][v].tolist()}
                self.events.append(("keep_strings", v, used))


@pytest.mark.parametrize("seed", dm.SEEDS)
def test_model_equals_the_replayed_log(scripts, seed):
    sc = scripts[seed]
    model, log = dm.new_model(sc), Log(sc)
    for i, op in enumerate(sc["ops"]):
        before = model.snapshot()
        dm.apply(model, op)
        log.feed(op)
        keys, vocabs = log.replay()
        tag = (seed, i, dm.describe(op))
        assert model.raw_keys() == keys, tag
        assert [v.values for v in model.vocabs] == vocabs, tag
        # the codes a key holds name its strings' places in the vocabulary, and every id is its place in the list
        assert all(model.keys.index[k] == j for j, k in enumerate(model.keys.keys)), tag
        for check in op["checks"]:
            dm.apply(model, check)
        after = model.snapshot()
        assert after["values"] == vocabs and model.raw_keys() == keys, (tag, "a read-only check changed the model")
        if op["kind"] in ("lookup", "select", "decode", "restart", "refused"):
            assert before["values"] == after["values"] and before["num_keys"] == after["num_keys"], tag
            assert all(np.array_equal(x, y) for x, y in zip(before["key_cols"], after["key_cols"])), tag


def flat(x):
    """a script as nested plain values, arrays as (dtype, bytes)"""
    if isinstance(x, dict):
        return {str(k): flat(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [flat(v) for v in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x.item() if isinstance(x, np.generic) else x


@pytest.mark.parametrize("seed", (0, 1, 2, 3, 4, 17, 31))
def test_a_script_is_a_function_of_its_seed(scripts, seed):
    assert flat(dm.make_script(seed)) == flat(scripts[seed])
    assert len(scripts[seed]["ops"]) == dm.N_OPS and all(len(op["checks"]) == 2 for op in scripts[seed]["ops"])


# ---- 2. what the 32 seeds cover ----
def test_every_kind_and_every_refusal(scripts):
    kinds = collections.Counter(op["kind"] for _, _, op in ops_of(scripts))
    assert set(kinds) == set(dm.KINDS), kinds
    assert kinds["encode"] >= 100 and kinds["compact_keys"] >= 30 and kinds["retire_strings"] >= 30 and kinds["refused"] >= 32, kinds
    assert all(kinds[k] >= 12 for k in ("lookup", "select", "decode", "restart")), kinds
    checks = collections.Counter(op["kind"] for _, _, op in ops_of(scripts, checks=True))
    assert checks["lookup"] >= 32 * dm.N_OPS and all(checks[k] >= 60 for k in dm.CHECK_KINDS), checks
    refusals = collections.Counter(op["variant"] for _, _, op in ops_of(scripts, "refused"))
    assert set(refusals) == set(dm.REFUSALS) and min(refusals.values()) >= 2, refusals
    assert all(any(op["kind"] == "refused" for op in sc["ops"]) for sc in scripts)
    classes = collections.Counter(sc["class"] for sc in scripts)
    assert set(classes) == set(dm.CLASSES) and min(classes.values()) >= 6, classes


def test_batches_sides_memories_and_forms(scripts):
    for kind in ("encode", "lookup"):
        ops = [op for _, _, op in ops_of(scripts, kind, checks=True)]
        assert {op["sides"] for op in ops} == {1, 2}, kind
        assert {op["key_mem"] for op in ops} == {"host", "device"}, kind
        forms = [f for op in ops for f in op["forms"].values()]
        assert {(f["bits"], f["mem"], f["validity"]) for f in forms} == {(b, m, v) for b in (32, 64) for m in ("host", "device") for v in (False, True)}, kind
        assert {f["shift"] for f in forms if f["mem"] == "device"} >= set(range(0, 16)), kind
        assert any(op["keep_a"] is not None and not op["keep_a"].all() for op in ops) and any(op["keep_b"] is not None for op in ops), kind
        # nulls that still own bytes
        assert any(nulls is not None and any(z and len(s) for s, z in zip(strings, nulls)) for op in ops for side in op["strs"] for strings, nulls in side.values())
    enc = ops_of(scripts, "encode")
    capped = [op for _, _, op in enc if op["max_new"] is not None]
    assert len(capped) >= 8 and all(op["max_new"] < op["info"]["keys_after"] - op["info"]["keys_before"] for op in capped)
    assert sum(1 for _, _, op in enc if any(x is not None for x in op["str_max_new"].values())) >= 10
    # known, new and previously retired tuples in one batch; retired tuples among the rows of the lookups
    assert sum(1 for _, _, op in enc if 0 < op["info"]["keys_after"] - op["info"]["keys_before"] < op["n"] * op["sides"] and op["info"]["keys_before"]) >= 60
    assert sum(1 for _, _, op in ops_of(scripts, "lookup", checks=True) if op["retired_rows"]) >= 100


def test_selections_and_decodes(scripts):
    sel = [op for _, _, op in ops_of(scripts, "select", checks=True)]
    assert {len(op["terms"]) for op in sel} == {1, 2, 3} and {op["side"] for op in sel} == {None, 0, 1} and {op["mem"] for op in sel} == {"host", "device"}
    terms = [t for op in sel for t in op["terms"]]
    assert {(t["how"], t["op"], t["nocase"]) for t in terms} == {("match", dm.STR_EQUAL, False), ("match", dm.STR_CONTAINS_NOCASE, True), ("like", None, False),
                                                                ("like", None, True)}
    likes = [t["pattern"] for t in terms if t["how"] == "like"] + [op["pattern"] for _, _, op in ops_of(scripts, "like", checks=True)]
    assert all(sum(1 for p in likes if ch in p) >= 20 for ch in (b"%", b"_", b"\\")), "patterns with %, _ and \\"
    assert {(op["mem"], op["nocase"]) for _, _, op in ops_of(scripts, "like", checks=True)} == {(m, n) for m in ("host", "device") for n in (False, True)}
    dec = [op for _, _, op in ops_of(scripts, "decode", checks=True)]
    assert {op["mem"] for op in dec} == {"host", "device"} and {(op["mem"], op["strings_to"]) for op in dec} >= {("device", "host"), ("device", "device")}
    assert any(op["cols"] is None for op in dec) and any(op["cols"] is not None for op in dec)
    assert sum(1 for op in dec if np.unique(op["ids"]).size < op["ids"].size and (np.diff(op["ids"].astype(np.int64)) < 0).any()) >= 20, "repeats, any order"


def test_restarts_compactions_and_the_chain(scripts):
    rs = [op for _, _, op in ops_of(scripts, "restart")]
    assert any(op["slices"] is None for op in rs) and {op["slices"] for op in rs} >= {1, 7, 100}
    ck = [op for _, _, op in ops_of(scripts, "compact_keys")]
    assert {op["variant"] for op in ck} == set(dm.SURVIVORS) and {op["mem"] for op in ck} == {"host", "device"}
    assert any(op["info"]["keys_before"] > 0 and op["info"]["keys_after"] == 0 for op in ck), "a compaction to zero"
    assert any(op["info"]["keys_before"] > 0 and op["info"]["keys_after"] == op["info"]["keys_before"] for op in ck), "a compaction of nothing"
    chain = ops_of(scripts, "retire_strings")
    assert {op["mem"] for _, _, op in chain} == {"host", "device"}
    assert any(b and a == [0] * len(a) for _, _, op in chain for b, a in [(sum(op["info"]["values_before"]), op["info"]["values_after"])]), "strings to zero"
    assert any(op["info"]["values_before"] == op["info"]["values_after"] and sum(op["info"]["values_before"]) for _, _, op in chain), "nothing retired"
    # the shared vocabulary: the second column's mark call adds to the first's; a superset keep: a value no key uses survives
    shared = superset = 0
    for sc, i, op in chain:
        model = dm.new_model(sc)
        for o in sc["ops"][:i]:
            dm.apply(model, o)
        out = dm.apply(model, op)
        shared += any(len(n) == 2 and n[1] > n[0] for n in out["n_used"].values())
        superset += any(out["stats"][v]["values_after"] > int(np.count_nonzero(out["used"][v])) for v in out["used"])
    assert shared >= 5 and superset >= 5, (shared, superset)
    assert sum(1 for sc, _, op in chain if sc["class"] == "wide" and op["mem"] == "device") >= 2


def test_the_shape_classes(scripts):
    by = collections.defaultdict(list)
    for sc in scripts:
        by[sc["class"]].append(sc)
    # 1. growth from the minimum sizes: table, records and arena grow several times, and each once more AFTER a compaction
    for sc in by["growth"] + by["churn"] + by["collide"]:
        assert sc["expected"] == (1, 1, 1)
    assert all(len(sc["str_cols"]) == 1 and sc["n_cols"] == 3 for sc in by["growth"])
    last = [sc["ops"][-1]["info"] for sc in by["growth"]]
    assert max(x["max_keys"] for x in last) >= 4500 and max(x["max_values"] for x in last) >= 1700, last
    assert all(200 <= op["n"] <= 3000 for sc in by["growth"] for op in sc["ops"] if op["kind"] == "encode")
    for sc in by["growth"]:
        grew = collections.Counter(g for op in sc["ops"] for g in op["info"]["grew"])
        assert all(grew[g] >= 2 for g in ("keys_table", "keys_records", "values_table", "values_records", "values_arena")), (sc["seed"], grew)
    after = collections.Counter(g for sc in scripts for op in sc["ops"] for g in op["info"]["grew_after_compaction"])
    assert all(after[g] >= 5 for g in ("keys_table", "keys_records", "values_table", "values_records", "values_arena")), after
    # 2. wide and two-sided: eight columns, three of them strings, two of which share a vocabulary
    for sc in by["wide"]:
        assert sc["n_cols"] == 8 and sorted(sc["str_cols"].values()) == [0, 0, 1] and sc["ops"][-1]["info"]["max_keys"] <= 600
        assert all(op["sides"] == 2 for op in sc["ops"] if op["kind"] == "encode")
    # 3. long strings: every length held at the moment of a decode and of a string compaction
    assert all(sc["ops"][-1]["info"]["max_values"] <= 300 for sc in by["long"])
    for kind in ("decode", "retire_strings"):
        held = {n for sc in by["long"] for op in sc["ops"] for o in [op] + op["checks"] if o["kind"] == kind for n in o["info"]["lengths_held"]}
        assert held >= set(dm.LONG_LENGTHS), (kind, sorted(set(dm.LONG_LENGTHS) - held))
    # 4. churn: grow, compact the keys to under a quarter, retire strings, grow past the old maximum, restart — the chain at least twice
    for sc in by["churn"]:
        kinds = [op["kind"] for op in sc["ops"]]
        chains = [i for i in range(len(kinds) - 2) if kinds[i:i + 3] == ["compact_keys", "retire_strings", "encode"]]
        assert len(chains) >= 2 and "restart" in kinds[chains[0]:chains[1]], (sc["seed"], kinds)
        for i in chains:
            ck, rt, en = (sc["ops"][j]["info"] for j in (i, i + 1, i + 2))
            assert ck["keys_after"] * 4 < ck["keys_before"], (sc["seed"], i)
            assert sum(rt["values_after"]) * 2 < sum(rt["values_before"]), (sc["seed"], i)
            assert en["keys_after"] > ck["max_keys"] and max(en["values_after"]) > rt["max_values"], (sc["seed"], i, "past the old maximum")
    # 5. engineered collisions: a same-fingerprint pair and a cluster that wraps the last slot, of tuples and of strings, held while a
    # growth, a key compaction and the retire chain (string compaction + recode) re-place them
    assert len(by["collide"]) >= 2
    for sc in by["collide"]:
        model = dm.new_model(sc)
        for i, op in enumerate(sc["ops"][:4]):
            dm.apply(model, op)
            keys, values = model.keys.keys, model.vocabs[0].values
            assert model.vocabs[0].values[0] == dm.ANCHOR
            assert dm.same_fingerprint_pair(keys[:8]) and dm.wrapping_cluster(keys[:8]), (sc["seed"], i, "tuples")
            assert dm.same_fingerprint_pair(values[:8]) and dm.wrapping_cluster(values[:8]), (sc["seed"], i, "strings")
        assert [op["kind"] for op in sc["ops"][:4]] == ["encode", "encode", "compact_keys", "retire_strings"]
        first, second = sc["ops"][0]["info"], sc["ops"][1]["info"]
        assert first["keys_after"] <= 32 and max(first["values_after"]) <= 32, "the engineered keys meet in the 64-slot tables"
        assert not {"keys_table", "values_table", "keys_records", "values_records"} & set(first["grew"])
        assert {"keys_table", "values_table"} <= set(second["grew"])
