"""GPU: seeded sequences of operations on a key dictionary and the string dictionaries of its string columns against a host model of
both (tests/dict_model.py).

include/tad.h defines every dictionary call as a function of what the dictionary holds — the values in code order, the (side, tuple)
keys in id order — so the reference side is two Python lists and the rules restated over them: no engine call, no twin dictionary, no
hash.  A script (dict_model.make_script) mixes batches that go through the vocabularies and then through the key dictionary (32- and
64-bit offsets, validity bitmaps whose nulls own bytes, host and device memory, device slices at odd byte offsets, one- and two-sided,
keep masks, capped new_first_row lists), read-only lookups, key selections from match and like masks, gathers with decodes, restarts
through export / import, key compactions, the whole string-retire chain (mark with accumulate, compact, ONE recode) and calls that
must be refused, over five shape classes: growth from the minimum sizes, eight columns with a shared vocabulary and two-sided batches,
long strings, churn, and engineered hash collisions.  After EVERY operation: the call's own outputs equal the model's; the whole
content (every tuple and side, every vocabulary's values, the counts) equals the model's; two read-only checks — a mixed lookup with
retired tuples among its rows, and one of select / gather + decode / like — return what the model returns and leave the content as it
was.  Everything is compared bit for bit; there is no tolerance in this file.  nbytes() is not modelled: it must be unchanged by
read-only and refused calls and must not grow in a compaction, which is all tad.h promises.

What the seed set covers is asserted on the host by tests/test_dict_model.py.  A failure names (seed, operation index, kind,
arguments); replay(engine, seed, upto) below rebuilds the dictionaries as they were before operation `upto`.

Time.  The reference side was measured once per seed on one host core without a device: building the script, the model's steps, every
expected output and the second formulation of tests/test_dict_model.py take at most 0.5 s of a seed (seed 4, the first collide seed:
it runs the collision searches, which later seeds reuse; 0.4 s for the growth seeds 10 and 20 and the long-string seed 7; 5.7 s for
all 32), against the 0.8 s / 6.4 s of the state sequences' reference side.  On an MI355X the 32 seeds take 4.3 s together, the slowest
(seeds 25, 23 and 5, growth and churn) 0.5 s."""
import pytest

import dict_model as dm
from dict_drivers import assert_outputs, assert_snapshot, execute, new_dicts, run_check, snapshot
from theia_amd import TadError

pytestmark = pytest.mark.gpu

READ_ONLY = ("lookup", "select", "decode", "like", "refused")


def replay(engine, seed, upto):
    """-> (dictionaries, model, script) as they are before operation `upto` of the seed's script; nothing is compared on the way"""
    sc = dm.make_script(seed)
    dicts, model = new_dicts(engine, sc), dm.new_model(sc)
    for op in sc["ops"][:upto]:
        dicts, _ = execute(engine, dicts, sc, op)
        dm.apply(model, op)
    return dicts, model, sc


@pytest.mark.parametrize("seed", dm.SEEDS)
def test_sequence(engine, seed):
    sc = dm.make_script(seed)
    dicts, model = new_dicts(engine, sc), dm.new_model(sc)
    for i, op in enumerate(sc["ops"]):
        tag = (seed, i, op["kind"], dm.describe(op))
        held = dicts.nbytes()
        try:
            dicts, got = execute(engine, dicts, sc, op)
        except TadError as exc:
            raise AssertionError((tag, "the call failed", str(exc)))
        want = dm.apply(model, op)
        # 1. the call's own outputs
        assert_outputs(got, want, tag)
        # 2. the whole content
        expected = model.snapshot()
        assert_snapshot(snapshot(dicts), expected, (tag, "content"))
        now = dicts.nbytes()
        if op["kind"] in READ_ONLY:
            assert now == held, (tag, "nbytes changed", held, now)
        if op["kind"] in ("compact_keys", "retire_strings"):
            assert all(n <= h for n, h in zip(now, held)), (tag, "nbytes grew in a compaction", held, now)
        # 3. two read-only checks
        for check in op["checks"]:
            ctag = (tag, "check", check["kind"], dm.describe(check))
            assert_outputs(run_check(engine, dicts, sc, check), dm.apply(model, check), ctag)
        assert_snapshot(snapshot(dicts), expected, (tag, "content after the read-only checks"))
        assert dicts.nbytes() == now, (tag, "nbytes changed in the read-only checks", now, dicts.nbytes())
    dicts.close()
