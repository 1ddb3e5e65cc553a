"""The host model of tad_state_rollup (include/tad.h) and seeded operation scripts that mix roll-ups into those of tests/state_model.py —
a helper module, no tests in it.

RollupModel is StateModel plus rollup(): the bound floored to a bucket start, every time below it replaced by its bucket's start (numpy's
floor division), then Stage 0 of the oracle over the result — the header's words, nothing of the kernels.  expected_snapshot() then gives
what the state must hold.  make_script(seed) is state_model's generator with roll-ups drawn into every script; tests/test_rollup_model.py
checks model and seeds on the host, tests/test_gpu_rollup_sequences.py runs the scripts on a state."""
import numpy as np

from oracle import tad_oracle as orc

import state_model as sm
from state_model import HIST, I64, SER, TIMES, U64, StateModel

STATS = ("points_before", "points_after", "points_rolled", "buckets", "keys_changed", "before_t")
SEEDS = tuple(range(8))


def bucket_start(t, bucket_s, origin=0):
    t = np.asarray(t, I64)
    return I64(origin) + I64(bucket_s) * ((t - I64(origin)) // I64(bucket_s))


class RollupModel(StateModel):
    def rollup(self, before, bucket_s, origin=0, op=None):
        """tad_state_rollup.  Returns the counters of tad_rollup_stats."""
        op = op or self.op
        k, t, v = self.points()
        b = int(bucket_start(before, bucket_s, origin))
        below = t < b
        t2 = np.where(below, bucket_start(t, bucket_s, origin), t)
        n0 = np.bincount(k.astype(I64), minlength=self.num_keys)
        out = {"points_before": int(k.size), "points_after": int(k.size), "points_rolled": 0, "buckets": 0, "keys_changed": 0, "before_t": b}
        if not below.any():
            return out
        nk, nt, nv = orc.stage0(k, t2, v, op)
        self._set(nk, nt, nv)
        n1 = np.bincount(nk.astype(I64), minlength=self.num_keys)
        out.update(points_after=int(nk.size), points_rolled=int(below.sum()), buckets=int((nt < b).sum()), keys_changed=int((n1 < n0).sum()))
        return out

    def lost_a_point(self, before, bucket_s, origin=0):
        """mask over the keys: the roll-up would fold at least two of the key's points into one"""
        k, t, _ = self.points()
        b = int(bucket_start(before, bucket_s, origin))
        t2 = np.where(t < b, bucket_start(t, bucket_s, origin), t)
        dup = np.zeros(k.size, bool)
        dup[1:] = (k[1:] == k[:-1]) & (t2[1:] == t2[:-1])
        return np.bincount(k[dup].astype(I64), minlength=self.num_keys) > 0


def apply(model, op, rows=True):
    """state_model.apply with the roll-up"""
    if op["kind"] == "rollup":
        return {"stats": model.rollup(op["before"], op["bucket_s"], op["origin"], op["op"])}
    return sm.apply(model, op, rows)


class _RollupGen(sm._Gen):
    """state_model's draws with roll-ups drawn into the plan; the model is a RollupModel"""

    def __init__(self, seed):
        super().__init__(seed)
        self.m = RollupModel(self.K0, self.flags, self.op, self.alpha)
        self.tiers = []

    def rollup(self):
        rng = self.rng
        variant = str(rng.choice(["old", "old", "most", "all", "again", "coarser", "nothing"]))
        bucket_s = int(rng.choice([2, 5, 60]) * self.step)
        origin = int(rng.choice([0, bucket_s // 3]))
        before = self.quantile_time({"old": 0.4, "most": 0.85}.get(variant, 0.5))
        if variant == "all":                                   # every key wholly below the bound: every last_t moves
            before = int(self.time_of(self.cursor + 2 * 60))
        if variant == "nothing":
            before = int(self.m.t.min()) - 7 * bucket_s if self.m.t.size else 0
        if variant in ("again", "coarser") and self.tiers:    # the last tier once more / at a multiple of its bucket with a congruent origin
            before, bucket_s, origin = self.tiers[-1]
            if variant == "coarser":
                origin, bucket_s = origin, bucket_s * int(rng.choice([2, 3, 10]))
        self.tiers.append((before, bucket_s, origin))
        return dict(kind="rollup", before=before, bucket_s=bucket_s, origin=origin, op=self.op, variant=variant)

    def plan(self):
        kinds = super().plan()
        free = [i for i, kd in enumerate(kinds) if i >= 1 and kd not in ("refused", "hard_trim", "compact_unseen", "resize_back")]
        for i in self.rng.choice(free, size=min(4, len(free)), replace=False):
            kinds[int(i)] = "rollup"
        return kinds

    def script(self):
        ops = []
        for kind in self.plan():
            m = self.m
            if m.num_keys * 2 < self.K0 and kind != "resize_back":
                kind = "resize_back"
            op = self.draw(kind)
            n0, _ = m.per_key()
            held0 = m.key.size
            out = apply(m, op, rows=False)
            op["info"] = info = {"held_before": int(held0), "keys_before": int(n0.size)}
            if op["kind"] in ("append", "merge") and op["k"].size:
                self.cursor = max(self.cursor, int((op["t"].max() - self.t_base) // self.step) + 1)
                self.last_batch = (op["k"], op["t"], op["v"])
            if op["kind"] in ("merge", "compact", "rollup"):
                info.update(out["stats"])
            if op["kind"] == "trim":
                info.update(dropped=out["dropped"])
            if op["kind"] == "compact":
                self.last_batch = None
            info["held_after"] = int(m.key.size)
            assert m.key.size <= sm.CEILING
            op["checks"] = self.checks()
            ops.append(op)
        return ops


def make_script(seed):
    g = _RollupGen(seed)
    ops = g.script()
    return {"seed": seed, "class": g.cls, "num_keys": g.K0, "flags": g.flags, "op": g.op, "alpha": g.alpha, "ops": ops}
