"""The host model of tad_state_replace (include/tad.h) on top of tests/state_model.py, and seeded scripts that mix replaces with the other
calls on a state — a helper module, no tests in it.

ReplaceModel.replace is the header's W' rule in numpy: W' = {w in W : time(w) not in R and (key, time)(w) not a point of B} ++ B, with B
Stage 0's points of the batch without the ones under keep_from and R the half-open range of a ranged call.  The counters of
tad_replace_stats are restated from sets of (key, time).  What the state must hold afterwards is StateModel.expected_snapshot over W':
the stream oracle on a fresh state, no engine call.

make_script(seed) is state_model's generator, driven through a subclass that draws a replace where the parent draws nothing of the kind;
everything else (appends, late batches, merges, trims, compactions, resizes, restarts, refusals, the read-only checks and the ARIMA
limits: series <= 40 points, <= 3 checks per script) is the parent's."""
import numpy as np

from oracle import tad_oracle as orc

import state_model as sm
from state_model import I64, U64, StateModel, _cat, _member

SEEDS = tuple(range(8))
REPLACE_VARIANTS = ("plain", "range", "range", "from_only", "to_only", "everything", "empty_range", "beyond", "resend", "reread", "empty_batch", "keep")
COUNTERS = ("batch_points", "points_too_old", "points_appended", "points_inserted", "points_replaced", "points_erased", "keys_emptied")


def in_range(t, from_t, to_t, ranged):
    """R of the header: empty without the flag; 0 = no bound on that side; half-open"""
    if not ranged:
        return np.zeros(np.asarray(t).size, bool)
    m = np.ones(np.asarray(t).size, bool)
    if from_t:
        m &= t >= from_t
    if to_t:
        m &= t < to_t
    return m


class ReplaceModel(StateModel):
    def replace(self, k, t, v, from_t=0, to_t=0, ranged=False, keep_from=0):
        """tad_state_replace.  Returns the tad_replace_stats counters."""
        k, t, v = np.asarray(k, U64), np.asarray(t, I64), np.asarray(v, U64)
        bk, bt, bv = orc.stage0(k, t, v, self.op) if k.size else sm._empty()
        counts = {"rows_in": int(k.size), "rows_used": int(k.size), "batch_points": int(bk.size)}
        if keep_from:
            keep = bt >= keep_from
            counts["points_too_old"] = int((~keep).sum())
            bk, bt, bv = bk[keep], bt[keep], bv[keep]
        else:
            counts["points_too_old"] = 0
        wk, wt, wv = self.points()
        n0, last = self.per_key()
        named = _member(wk, wt, bk, bt)                       # old points the batch names: they take its value
        erased = in_range(wt, from_t, to_t, ranged) & ~named   # old points of R it does not name
        bi = bk.astype(I64)
        newer = (n0[bi] == 0) | (bt > last[bi])
        counts["points_replaced"] = int(named.sum())
        counts["points_appended"] = int(newer.sum())
        counts["points_inserted"] = int(bk.size) - counts["points_replaced"] - counts["points_appended"]
        counts["points_erased"] = int(erased.sum())
        if bk.size or erased.any():
            keep_old = ~named & ~erased
            # (no (key, time) is left twice: the aggregation only sorts)
            self._set(*orc.stage0(*_cat((wk[keep_old], wt[keep_old], wv[keep_old]), (bk, bt, bv)), self.op))
        n1, _ = self.per_key()
        counts["keys_emptied"] = int(((n0 > 0) & (n1 == 0)).sum())
        return counts


def apply(model, op, rows=True):
    """state_model.apply, and the replace"""
    if op["kind"] == "replace":
        return {"stats": model.replace(op["k"], op["t"], op["v"], op["from_t"], op["to_t"], op["ranged"], op["keep_from"])}
    return sm.apply(model, op, rows)


class _Gen(sm._Gen):
    def __init__(self, seed):
        super().__init__(seed)
        self.m = ReplaceModel(self.m.num_keys, self.flags, self.op, self.alpha)

    def plan(self):
        kinds = super().plan()
        rng = self.rng
        at = [i for i, kd in enumerate(kinds) if kd not in ("refused", "append_few", "append_all", "hard_trim", "compact_unseen", "resize_back") and i > 0]
        for i in rng.choice(at, size=min(len(at), 4 + int(rng.integers(2))), replace=False):
            kinds[int(i)] = "replace"
        return kinds

    def replace(self):
        rng, m = self.rng, self.m
        variant = str(rng.choice(REPLACE_VARIANTS))
        if variant == "resend" and self.last_batch is None:
            variant = "range"
        from_t = to_t = keep_from = 0
        ranged = variant != "plain"
        if variant == "resend":
            rows = self.last_batch
            from_t, to_t = int(rows[1].min()), int(rows[1].max()) + 1
        elif variant == "reread":
            # every row of W from a drawn time on, each point once, some of the values changed: the poll loop's batch
            from_t = self.quantile_time(float(rng.choice([0.5, 0.8, 0.95])))
            sel = m.t >= from_t
            k, t, v = m.key[sel], m.t[sel], m.value[sel].copy()
            ch = rng.random(k.size) < 0.3
            v[ch] = self.values(k[ch])
            o = rng.permutation(k.size)
            rows = (k[o], t[o], v[o])
        elif variant == "empty_batch":
            rows = sm._empty()
            from_t, to_t = self.quantile_time(0.6), self.quantile_time(0.9)
        else:
            mop = self.merge("range_keep" if variant == "keep" else "range")
            if mop["kind"] != "merge":
                return mop
            rows = (mop["k"], mop["t"], mop["v"])
            keep_from = mop["keep_from"]
            if variant in ("range", "keep"):
                from_t = self.quantile_time(float(rng.choice([0.0, 0.3, 0.6])))
                to_t = max(from_t, self.quantile_time(float(rng.choice([0.7, 0.9, 1.0]))) + int(rng.integers(2)))
            elif variant == "from_only":
                from_t = self.quantile_time(float(rng.choice([0.5, 0.9])))
            elif variant == "to_only":
                to_t = self.quantile_time(float(rng.choice([0.1, 0.4])))
            elif variant == "empty_range":
                from_t = to_t = self.quantile_time(0.5)
            elif variant == "beyond":
                from_t = int(self.time_of(self.cursor + 50))
                to_t = from_t + 1000
        return self.batch_op("replace", rows, from_t=from_t, to_t=to_t, ranged=ranged, keep_from=keep_from, variant=variant)

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
            if op["kind"] in ("append", "merge", "replace") and op["k"].size:
                self.cursor = max(self.cursor, int((op["t"].max() - self.t_base) // self.step) + 1)
                self.last_batch = (op["k"], op["t"], op["v"])
            if op["kind"] in ("merge", "replace"):
                info.update(out["stats"])
            if op["kind"] == "compact":
                self.last_batch = None
            info["held_after"] = int(m.key.size)
            assert m.key.size <= sm.CEILING
            if self.cls == "arima":
                assert m.per_key()[0].max(initial=0) <= sm.ARIMA_MAX_SERIES + 8
            op["checks"] = self.checks()
            ops.append(op)
        return ops


def make_script(seed):
    """-> state_model.make_script's dictionary, with replaces among the operations; a function of the seed alone"""
    g = _Gen(1000 + seed)
    ops = g.script()
    return {"seed": seed, "class": g.cls, "num_keys": g.K0, "flags": g.flags, "op": g.op, "alpha": g.alpha, "ops": ops}
