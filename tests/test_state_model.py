"""The host model of the streaming-state API (tests/state_model.py) checked on the host: against a second formulation of what a state
holds, for what its seed set covers, and for determinism.  tests/test_gpu_state_sequences.py runs the same scripts on a device; a gap in
the scripts is a gap there, so the coverage conditions below are asserted, not measured."""
import numpy as np
import pytest

from oracle import stream_oracle as sorc
from oracle import tad_oracle as orc

import state_model as sm
from state_helpers import ROW_FIELDS

U64, I64 = np.uint64, np.int64


@pytest.fixture(scope="module")
def scripts():
    return [sm.make_script(seed) for seed in sm.SEEDS]


def ops_of(scripts, kind=None):
    return [(sc, i, op) for sc in scripts for i, op in enumerate(sc["ops"]) if kind is None or op["kind"] == kind]


# ---- 1. the model against a second formulation: every raw row ever fed, with an alive flag ----
class AliveRows:
    def __init__(self, num_keys, op):
        self.K, self.op = num_keys, op
        self.k, self.t, self.v, self.alive = np.zeros(0, U64), np.zeros(0, I64), np.zeros(0, U64), np.zeros(0, bool)

    def feed(self, k, t, v, keep_from=0):
        self.k, self.t, self.v = np.concatenate([self.k, k]), np.concatenate([self.t, t]), np.concatenate([self.v, v])
        self.alive = np.concatenate([self.alive, t >= keep_from if keep_from else np.ones(k.size, bool)])      # a merge's own old rows

    def times(self):
        """{key: ascending distinct times of its alive rows}"""
        out = {}
        for k, t in sorted(set(zip(self.k[self.alive].tolist(), self.t[self.alive].tolist()))):
            out.setdefault(k, []).append(t)
        return out

    def kill(self, dead):
        """dead: set of (key, time) points whose rows die"""
        if dead:
            self.alive &= np.array([(k, t) not in dead for k, t in zip(self.k.tolist(), self.t.tolist())], bool)

    def trim(self, keep_points, keep_from):
        dead = set()
        for k, ts in self.times().items():
            kept = [t for t in ts if not keep_from or t >= keep_from]
            kept = kept[-keep_points:] if keep_points else kept
            dead |= {(k, t) for t in ts if t not in set(kept)}
        self.kill(dead)
        return len(dead)

    def compact(self, retire_before):
        times = self.times()
        survivors = [k for k in range(self.K) if k in times and (not retire_before or times[k][-1] >= retire_before)]
        new_id = {k: j for j, k in enumerate(survivors)}
        self.kill({(k, t) for k, ts in times.items() if k not in new_id for t in ts})
        self.k = np.array([new_id.get(k, 0) for k in self.k.tolist()], U64)           # (dead rows keep any id: they are never read)
        self.K = max(len(survivors), 1)

    def points(self):
        return orc.stage0(self.k[self.alive], self.t[self.alive], self.v[self.alive], self.op)


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_model_equals_the_alive_raw_rows(scripts, seed):
    sc = scripts[seed]
    model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    rows = AliveRows(sc["num_keys"], sc["op"])
    for i, op in enumerate(sc["ops"]):
        out = sm.apply(model, op, rows=False)
        kind = op["kind"]
        if kind == "append":
            rows.feed(op["k"], op["t"], op["v"])
        elif kind == "merge":
            rows.feed(op["k"], op["t"], op["v"], op["keep_from"])
        elif kind == "trim":
            assert rows.trim(op["keep_points"], op["keep_from"]) == out["dropped"], (seed, i, sm.describe(op))
        elif kind == "compact":
            rows.compact(op["retire_before"])
        elif kind == "resize":
            rows.K = op["n"]
        assert rows.K == model.num_keys, (seed, i, sm.describe(op))
        for got, want in zip(model.points(), rows.points()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (seed, i, sm.describe(op))
        # every read-only check's window, by a loop over the keys
        for check in op["checks"]:
            f, t, kp = check.get("win", (0, 0, 0))
            want = np.zeros(model.key.size, bool)
            for k in np.unique(model.key):
                idx = [j for j in np.flatnonzero(model.key == k) if (not f or model.t[j] >= f) and (not t or model.t[j] < t)]
                want[idx[-kp:] if kp else idx] = True
            if check.get("mask") is not None:
                want &= check["mask"][model.key.astype(I64)] != 0
            assert np.array_equal(model.check_mask(check), want), (seed, i, check["call"], check.get("win"))


def test_the_emit_all_stream_rows_hold_the_stream_oracles_rows(scripts):
    """the model's per-point form of an EWMA stream batch (emit_all) against the stream oracle itself: same anomalous rows, and the
    oracle's state after the batch is the one-batch state over W"""
    seen = 0
    for sc in scripts:
        model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
        for op in sc["ops"]:
            if op["kind"] == "append" and op["algo"] == "EWMA" and model.key.size + op["k"].size < 4000 and seen < 12:
                before = model.expected_snapshot()["state"]
                pts = model.append(op["k"], op["t"], op["v"])
                every = model.ewma_stream_rows(before, *pts, True)
                some = model.ewma_stream_rows(before, *pts, False)
                a = every["anomaly"].astype(bool)
                for f in ROW_FIELDS:
                    assert np.array_equal(every[f][a].view(U64), some[f].view(U64)), f
                st = sorc.StreamState(model.num_keys)
                for f in sm.STATE_FIELDS:
                    getattr(st, f)[:] = before[f]
                st.seen[:] = before["n"] > 0
                sorc.run_stream(st, *pts, op=sc["op"], alpha=model.alpha_eff)
                after = model.expected_snapshot()["state"]
                for f in sm.STATE_FIELDS:
                    assert np.array_equal(getattr(st, f).view(U64) if f != "n" else st.n, after[f].view(U64) if f != "n" else after[f]), f
                seen += 1
            else:
                sm.apply(model, op, rows=False)
    assert seen == 12


# ---- 2. what the seed set covers, from the scripts alone ----
def test_every_operation_kind_and_refusal(scripts):
    for kind in sm.KINDS:
        assert len(ops_of(scripts, kind)) >= 10, kind
    for variant in sm.REFUSALS:
        assert sum(op["variant"] == variant for _, _, op in ops_of(scripts, "refused")) >= 2, variant
    for variant in ("eq", "lt"):
        assert sum(op["variant"] == variant for _, _, op in ops_of(scripts, "late")) >= 2, variant
    assert all(len(sc["ops"]) == sm.N_OPS for sc in scripts)
    assert all(op["info"]["held_after"] <= sm.CEILING for _, _, op in ops_of(scripts))


def test_merges(scripts):
    merges = [op for _, _, op in ops_of(scripts, "merge")]
    for f in ("points_inserted", "points_combined", "points_too_old", "points_appended"):
        assert sum(op["info"][f] > 0 for op in merges) >= 5, f
    assert sum(op["info"]["keys_replayed"] == 0 and op["info"]["keys_touched"] > 0 for op in merges) >= 3
    for variant in ("range", "range_keep", "resend", "inorder", "inorder_keep"):
        assert any(op["variant"] == variant for op in merges), variant
    assert any(op["keep_from"] for op in merges) and any(not op["keep_from"] for op in merges)


def test_trims(scripts):
    trims = [op for _, _, op in ops_of(scripts, "trim")]
    assert sum(op["info"]["dropped"] > 0 for op in trims) >= 10
    assert sum(op["info"]["keys_emptied"] > 0 for op in trims) >= 3
    assert sum(op["info"]["dropped"] == 0 for op in trims) >= 1
    for by_time in (False, True):
        for by_count in (False, True):
            assert any(bool(op["keep_from"]) == by_time and bool(op["keep_points"]) == by_count for op in trims), (by_time, by_count)


def test_compactions(scripts):
    info = [op["info"] for _, _, op in ops_of(scripts, "compact")]
    assert sum(c["keys_idle"] > 0 and c["points_dropped"] > 0 for c in info) >= 5
    assert sum(c["keys_idle"] == 0 and c["keys_unseen"] > 0 for c in info) >= 3
    assert sum(c["keys_idle"] == 0 and c["keys_unseen"] == 0 for c in info) >= 1
    assert sum(c["keys_after"] == 0 for c in info) >= 1
    assert any(op["retire_before"] for _, _, op in ops_of(scripts, "compact")) and any(not op["retire_before"] for _, _, op in ops_of(scripts, "compact"))


def test_windows(scripts):
    checks = [c for _, _, op in ops_of(scripts) for c in op["checks"] if c["call"] != "run_state"]
    assert sum(c["info"]["cut"] for c in checks) >= 10
    assert sum(c["info"]["whole"] for c in checks) >= 5
    dbscan = [c["info"] for c in checks if c["call"] == "window" and c["algo"] == "DBSCAN" and c["info"]["cut"]]
    assert sum(2 * c["window_points"] <= c["state_points"] for c in dbscan) >= 3          # the window's values are sorted
    assert sum(2 * c["window_points"] > c["state_points"] for c in dbscan) >= 3           # the excluded values leave the history
    masks = [c for c in checks if c["call"].endswith("keys")]
    assert any(c["mask_kind"] == "zeros" for c in masks) and any(c["mask_kind"] == "ones" for c in masks)
    for call in ("window", "keys", "drop_state", "drop_state_keys"):
        assert sum(c["call"] == call for c in checks) >= 10, call
    assert any(c["win"][0] and c["win"][0] == c["win"][1] for c in checks)                # from_t == to_t: an empty window


def test_shapes(scripts):
    for cls in sm.CLASSES:
        assert sum(sc["class"] == cls for sc in scripts) >= 4, cls
    for op in ("sum", "max"):
        assert sum(sc["op"] == op for sc in scripts) >= 8, op
    assert sum(bool(sc["flags"] & sm.HIST) for sc in scripts) >= 8 and sum(not sc["flags"] & sm.HIST for sc in scripts) >= 8
    assert sum(bool(sc["flags"] & sm.HIST) for sc in scripts) == 3 * len(scripts) // 4
    appends = [op for _, _, op in ops_of(scripts, "append")]
    for algo in ("EWMA", "DBSCAN", "ARIMA", "DROP"):
        assert sum(op["algo"] == algo for op in appends) >= 6, algo
    for emit_all in (False, True):
        assert sum(op["emit_all"] == emit_all for op in appends) >= 6
    for cols in ("host8", "host4", "device"):
        assert sum(op.get("cols") == cols for _, _, op in ops_of(scripts)) >= 6, cols
    for sparse in ("auto", "always", "never"):
        assert sum(op.get("plan", {}).get("sparse") == sparse for _, _, op in ops_of(scripts)) >= 6, sparse
    many = {sc["num_keys"] for sc in scripts if sc["class"] == "many"}
    assert many & {63, 64, 65} and many & {700, 3000}
    per_key = [np.bincount(op["k"].astype(I64)).max() for sc, _, op in ops_of(scripts, "append") if sc["class"] == "few-long"]
    assert min(per_key) <= 256 and any(256 < n <= 512 for n in per_key) and max(per_key) > 512      # both sides of 256 and of 512 points per key
    assert any(int(op["v"].max()) >= 1 << 50 for op in appends) and any(int(op["v"].max()) <= 1 << 31 for op in appends)
    arima = sum(c["algo"] == "ARIMA" for sc in scripts for op in sc["ops"] for c in op["checks"])
    assert arima >= 4
    for sc in scripts:
        n = sum(c["algo"] == "ARIMA" for op in sc["ops"] for c in op["checks"]) + sum(op.get("algo") == "ARIMA" for op in sc["ops"])
        assert n <= sm.MAX_ARIMA_CHECKS and (n == 0 or sc["class"] == "arima"), sc["seed"]


def test_grow_shrink_grow(scripts):
    """the class's forced part: a trim that keeps under a quarter of the points, a compaction after it, appends past the earlier maximum"""
    for sc in scripts:
        if sc["class"] != "grow-shrink-grow":
            continue
        ops = sc["ops"]
        hard = next(i for i, op in enumerate(ops) if op["kind"] == "trim" and 4 * op["info"]["held_after"] < op["info"]["held_before"])
        comp = next(i for i, op in enumerate(ops) if i > hard and op["kind"] == "compact")
        assert ops[comp]["info"]["keys_unseen"] > 0, sc["seed"]
        before = max(op["info"]["held_after"] for op in ops[:hard])
        assert max(op["info"]["held_after"] for op in ops[comp:] if op["kind"] == "append") > before, sc["seed"]
        assert any(op["kind"] == "append" and np.bincount(op["k"].astype(I64), minlength=1).size > ops[comp]["info"]["keys_after"] for op in ops[comp:])


# ---- 3. a script is a function of its seed ----
def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("seed", sm.SEEDS[::5])
def test_a_script_is_a_function_of_its_seed(scripts, seed):
    again = sm.make_script(seed)
    assert same(scripts[seed], again)
    assert not same(scripts[seed], scripts[(seed + 1) % len(scripts)])
