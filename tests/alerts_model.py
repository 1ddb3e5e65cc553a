"""The host model of the change report of tad_state_merge_changes / tad_state_replace_changes (include/tad.h: tad_changes) on top of
tests/state_model.py and tests/replace_model.py, which are imported and not edited — a helper module, no tests in it.

The report is the header's rule read literally: let W be the model's points() before the call and W' its points() after it; a point of
key k is changed iff it is in exactly one of W and W', or in both with different values; key_since[k] is the smallest changed time of key
k, NO_CHANGE where the key has none.  Nothing here knows how a merge or a replace works: the operation runs on the model, and the two
tables are compared."""
import numpy as np

import replace_model as rm
from state_model import I64, U64

NO_CHANGE = (1 << 63) - 1
COUNTERS = ("keys_changed", "points_changed", "min_t", "max_t")


def diff_points(before, after, num_keys):
    """the report of W = before -> W' = after, two (key, time, value) tables with one row per (key, time) -> {key_since: int64[num_keys],
    keys_changed, points_changed, min_t, max_t}"""
    (k0, t0, v0), (k1, t1, v1) = (tuple(np.asarray(a) for a in w) for w in (before, after))
    old = {(int(k), int(t)): int(v) for k, t, v in zip(k0.tolist(), t0.tolist(), v0.tolist())}
    new = {(int(k), int(t)): int(v) for k, t, v in zip(k1.tolist(), t1.tolist(), v1.tolist())}
    assert len(old) == k0.size and len(new) == k1.size, "a table holds a (key, time) twice"
    since = np.full(num_keys, NO_CHANGE, I64)
    changed = [p for p in old.keys() | new.keys() if old.get(p) != new.get(p)]   # (in one table only: None on the other side)
    for k, t in changed:
        since[k] = min(int(since[k]), t)
    times = [t for _, t in changed]
    return {"key_since": since, "keys_changed": int((since != NO_CHANGE).sum()), "points_changed": len(changed),
            "min_t": min(times) if times else 0, "max_t": max(times) if times else 0}


def _copy(points):
    return tuple(np.array(a, copy=True) for a in points)


class AlertsModel(rm.ReplaceModel):
    """ReplaceModel whose merge and replace also return the report under "changes" """

    def merge(self, k, t, v, keep_from=0):
        before = _copy(self.points())
        counts = super().merge(k, t, v, keep_from)
        counts["changes"] = diff_points(before, self.points(), self.num_keys)
        return counts

    def replace(self, k, t, v, from_t=0, to_t=0, ranged=False, keep_from=0):
        before = _copy(self.points())
        counts = super().replace(k, t, v, from_t, to_t, ranged, keep_from)
        counts["changes"] = diff_points(before, self.points(), self.num_keys)
        return counts


def apply_with_changes(model, op):
    """replace_model.apply for a merge or a replace of a script, run on any StateModel: -> (what apply returns, the report)"""
    before = _copy(model.points())
    out = rm.apply(model, op, rows=False)
    return out, diff_points(before, model.points(), model.num_keys)


def table(rows):
    """three lists -> a (key, time, value) table"""
    k, t, v = rows
    return np.array(k, U64), np.array(t, I64), np.array(v, U64)
