"""GPU: seeded sequences of operations on one streaming state against a host model of the whole state API (tests/state_model.py).

Every call on a state is defined by include/tad.h as a function of the table W of points the state holds, so the reference side is W
and the oracles alone: no engine call, no twin state.  A script (state_model.make_script) mixes stream batches of all four detectors,
refused late batches, merges (late, re-sent, in-order, with keep_from), trims, compactions, resizes, restarts through export / import
and calls that must be refused, over four shape classes; the columns are 8 or 4 bytes wide, on the host or the device, under the sparse
and both dense Stage 0.  After EVERY operation: the call's own outputs (rows, merge counters, points dropped, remap and compact
counters, num_keys) equal the model's; the whole state — moments, series, times, history — equals the model's expected snapshot; two
read-only jobs (run_state, and one of run_state_window / run_state_keys / drop_state / drop_state_keys over a drawn window and key
mask) return the oracle's rows and counters and leave the state as it was.  Everything is compared as bit patterns; there is no
tolerance in this file.

What the seed set covers is asserted on the host by tests/test_state_model.py.  A failure names (seed, operation index, kind,
arguments); replay(engine, seed, upto) below rebuilds the state as it was before operation `upto`.

Time.  The reference side was measured once per seed on one host core without a device: building the script, the model's steps, every
expected snapshot and every oracle job take at most 0.8 s of a seed (seeds 3, 28 and 29, the 700- and 3000-key states; 6.4 s for all
32), against a budget of 20 s per seed.  On an MI355X the 32 seeds take 5 s together, the slowest (seed 2, ARIMA) 0.45 s."""
import numpy as np
import pytest

import state_model as sm
from state_drivers import COMPACT_FIELDS, execute, run_check
from state_helpers import assert_counts, assert_rows, assert_same, bits, new_state, rows_of, snapshot

pytestmark = pytest.mark.gpu


def replay(engine, seed, upto):
    """-> (state, model, script) as they are before operation `upto` of the seed's script; nothing is compared on the way"""
    sc = sm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for op in sc["ops"][:upto]:
        st, _ = execute(engine, st, sc, op)
        sm.apply(model, op, rows=False)
    return st, model, sc


@pytest.mark.parametrize("seed", sm.SEEDS)
def test_sequence(engine, seed):
    sc = sm.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = sm.StateModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], sm.describe(op))
        st, got = execute(engine, st, sc, op)
        want = sm.apply(model, op)
        # 1. the call's own outputs
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        if "raises" in want:
            assert got["raises"], (tag, "the call must be refused")
        if "rows" in want:
            assert_rows(got["rows"], want["rows"], (tag, "rows"))
        if op["kind"] == "merge":
            assert_counts(got["stats"], want["stats"], tag)
        if "dropped" in want:
            assert got["dropped"] == want["dropped"], (tag, got["dropped"], want["dropped"])
        if "remap" in want:
            assert np.array_equal(bits(got["remap"]), bits(want["remap"])), (tag, "remap")
            for f in COMPACT_FIELDS:
                assert got["stats"][f] == want["stats"][f], (tag, f, got["stats"][f], want["stats"][f])
        assert st.num_keys == model.num_keys, (tag, st.num_keys, model.num_keys)
        # 2. the whole state
        expected = model.expected_snapshot()
        assert_same(snapshot(st), expected, (tag, "state"))
        # 3. two read-only jobs
        for check in op["checks"]:
            ctag = (tag, check["call"], check["algo"], check["emit_all"], check["params"], check.get("win"), check.get("mask_kind"))
            res = run_check(engine, st, check)
            rows, counters = model.check_expect(check)
            assert_rows(rows_of(res), rows, ctag)
            for f, v in counters.items():
                assert res.stats[f] == v, (ctag, f, res.stats[f], v)
            assert res.stats["rows_in"] == res.stats["rows_used"] == counters["n_points"], ctag
        assert_same(snapshot(st), expected, (tag, "state after the read-only jobs"))
    st.close()
