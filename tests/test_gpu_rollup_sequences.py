"""GPU: seeded sequences of operations with roll-ups among them, against the host model — tests/test_gpu_state_sequences.py with
tad_state_rollup drawn into every script (tests/rollup_model.py: the generator is state_model's, subclassed).  Roll-ups are mixed with
stream batches, refused late batches, merges, trims, compactions, resizes and restarts; after EVERY operation the call's own outputs equal
the model's, the whole state — moments, series, times, history — equals the model's expected snapshot, and two read-only jobs return the
oracle's rows and leave the state as it was.  A roll-up is made twice; the second call must change no bit.  Bit patterns only.
What the eight seeds cover is asserted on the host by tests/test_rollup_model.py."""
import numpy as np
import pytest

import rollup_model as R
import state_model as sm
from state_drivers import COMPACT_FIELDS, execute, run_check
from state_helpers import assert_counts, assert_rows, assert_same, bits, new_state, rows_of, snapshot

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", R.SEEDS)
def test_sequence_with_roll_ups(engine, seed):
    sc = R.make_script(seed)
    st = new_state(engine, sc["num_keys"], sc["flags"])
    model = R.RollupModel(sc["num_keys"], sc["flags"], sc["op"], sc["alpha"])
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], sm.describe(op))
        if op["kind"] == "rollup":
            args = (op["before"], op["bucket_s"], op["origin"], op["op"])
            got = {"stats": st.rollup(*args, alpha=sc["alpha"])}
        else:
            st, got = execute(engine, st, sc, op)
        want = R.apply(model, op)
        # 1. the call's own outputs
        assert set(got) == set(want), (tag, sorted(got), sorted(want))
        if "raises" in want:
            assert got["raises"], (tag, "the call must be refused")
        if "rows" in want:
            assert_rows(got["rows"], want["rows"], (tag, "rows"))
        if op["kind"] == "merge":
            assert_counts(got["stats"], want["stats"], tag)
        if op["kind"] == "rollup":
            for f in R.STATS:
                assert got["stats"][f] == want["stats"][f], (tag, f, got["stats"][f], want["stats"][f])
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
        if op["kind"] == "rollup":
            again = st.rollup(*args, alpha=sc["alpha"])
            assert again["keys_changed"] == 0 and again["points_after"] == again["points_before"], (tag, again)
            assert_same(snapshot(st), expected, (tag, "the second call changed a bit"))
        # 3. two read-only jobs
        for check in op["checks"]:
            ctag = (tag, check["call"], check["algo"], check["emit_all"], check["params"], check.get("win"), check.get("mask_kind"))
            res = run_check(engine, st, check)
            rows, counters = model.check_expect(check)
            assert_rows(rows_of(res), rows, ctag)
            for f, v in counters.items():
                assert res.stats[f] == v, (ctag, f, res.stats[f], v)
        assert_same(snapshot(st), expected, (tag, "state after the read-only jobs"))
    st.close()
