"""GPU: the two copies of a streaming state.  Everything a state holds is double-buffered and indexed by one `cur`; every state call
reads copy `cur`, writes the candidate `cur ^ 1` (or fresh memory) and decides which copy is current afterwards.  Two states with the
same content but OPPOSITE parity — A fed its rows as two batches (cur back at 0), B fed the same rows as one batch (cur == 1) — must
therefore stay indistinguishable through every call: a `[cur]`, `[cand]` or `[0]` in the wrong place shows as A != B or as a state that
differs from the references.  After each step both states take one more stream batch (which reads what the step left and commits
once more).  References: (R1) a fresh state streamed the surviving rows and the last batch as ONE batch; (R2) oracle/stream_oracle.py
over the same rows plus oracle.tad_oracle.stage0 for series, times and sorted history.  Everything is compared bit for bit; nbytes() is
not compared (capacities legitimately differ with parity)."""
import numpy as np
import pytest

from oracle import stream_oracle as sorc
from oracle import tad_oracle as orc
from state_helpers import SKIP, STATE_FIELDS, T_BASE, assert_same, bits, new_state, snapshot

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev", "anomaly")
K = 6
OP = "sum"


def at(i):
    return T_BASE + 60 * i


def table():
    """39 points, one row each and one point with two: key 0 unseen, key 1 a single point, key 2 idle after minute 5, key 3 long (no
    point at minute 7: the merge's late point), keys 4 and 5 short.  Returns (rows of minutes < 10, rows of minutes >= 10)."""
    minutes = {1: [15], 2: range(6), 3: [i for i in range(20) if i != 7], 4: range(1, 20, 2), 5: [2, 12, 13]}
    k = np.concatenate([np.full(len(m), key, np.uint64) for key, m in minutes.items()] + [np.array([4], np.uint64)])
    i = np.concatenate([np.asarray(list(m), np.int64) for m in minutes.values()] + [np.array([3], np.int64)])
    rng = np.random.default_rng(5)
    v = (1_000_000_000 + rng.integers(0, 2_000_000_000, size=k.size)).astype(np.uint64)
    order = rng.permutation(k.size)
    k, i, v = k[order], i[order], v[order]
    return (k[i < 10], at(i[i < 10]), v[i < 10]), (k[i >= 10], at(i[i >= 10]), v[i >= 10])


def last_batch(keys):
    """minutes 30-32 for every key of `keys`"""
    keys = np.asarray(keys, np.uint64)
    k = np.repeat(keys, 3)
    t = np.tile(at(np.arange(30, 33)), keys.size).astype(np.int64)
    v = (3_000_000_000 + 7_000_000 * np.arange(k.size)).astype(np.uint64)
    return k, t, v


def cat(*rows):
    return tuple(np.concatenate([r[c] for r in rows]) for c in range(3))


def pair(engine):
    """A (two batches, cur == 0) and B (one batch, cur == 1) over the same rows"""
    first, second = table()
    a, b = new_state(engine, K), new_state(engine, K)
    engine.run_stream(a, *first, value_op=OP)
    engine.run_stream(a, *second, value_op=OP)
    engine.run_stream(b, *cat(first, second), value_op=OP)
    assert_same(snapshot(a), snapshot(b), "before the step")
    return a, b, cat(first, second)


def oracle_snapshot(num_keys, rows):
    os_ = sorc.StreamState(num_keys)
    pk, pt, pv = orc.stage0(rows[0], rows[1], rows[2], OP)
    sorc.run_stream(os_, rows[0], rows[1], rows[2], op=OP, alpha=0.5)
    ln = np.bincount(pk.astype(np.int64), minlength=num_keys).astype(np.uint64)
    return {"state": {f: getattr(os_, f) for f in STATE_FIELDS}, "history": (ln, pv[np.lexsort((pv, pk))]), "series": (ln, pv), "times": pt}


def finish(engine, states, surviving, keys, what):
    """one more batch on every state; then all states are one another's equal, the fresh state's and the oracle's"""
    num_keys = states[0].num_keys
    batch = last_batch(keys)
    snaps, rows = [], []
    for st in states:
        assert st.num_keys == num_keys, what
        engine.run_stream(st, *batch, value_op=OP)
        snaps.append(snapshot(st))
        rows.append([engine.run_state(st, algo=algo, emit_all=True).to_host() for algo in ("EWMA", "DBSCAN", "ARIMA")])
    for i in range(1, len(states)):
        assert_same(snaps[0], snaps[i], (what, "A == B", i))
        for ra, rb in zip(rows[0], rows[i]):
            assert ra["key_id"].size == rb["key_id"].size > 0, (what, i)
            for f in ROW_FIELDS:
                assert np.array_equal(bits(ra[f]), bits(rb[f])), (what, "run_state", i, f)
    everything = cat(surviving, batch)
    ref = new_state(engine, num_keys)
    engine.run_stream(ref, *everything, value_op=OP)
    assert_same(snaps[0], snapshot(ref), (what, "a state built from scratch"))
    assert_same(snaps[0], oracle_snapshot(num_keys, everything), (what, "oracle"))
    for st in states + [ref]:
        st.close()


def test_resize(engine):
    a, b, rows = pair(engine)
    for st in (a, b):
        st.resize(K + 3)
    finish(engine, [a, b], rows, [1, 3, 4, 5, K + 1], "resize")


def test_export_and_import(engine):
    a, b, rows = pair(engine)
    sa, sb = snapshot(a), snapshot(b)
    copies = [new_state(engine, K), new_state(engine, K)]       # fresh states from either export ...
    for st, snap in zip([a, b] + copies, (sb, sa, sa, sb)):   # ... and each state takes the other's, into its own candidate copies
        st.load(snap["state"])
        st.load_history(*snap["history"])
        st.load_series(*snap["series"])
        st.load_times(snap["times"])
    finish(engine, [a, b] + copies, rows, [1, 3, 4, 5], "import")


def test_trim(engine):
    a, b, rows = pair(engine)
    for st in (a, b):
        assert st.trim(keep_points=3) == 39 - (1 + 3 + 3 + 3 + 3)
    pk, pt, pv = orc.stage0(*rows, OP)
    keep = np.zeros(pk.size, bool)
    for key in np.unique(pk):
        keep[np.flatnonzero(pk == key)[-3:]] = True
    finish(engine, [a, b], (pk[keep], pt[keep], pv[keep]), [1, 3, 4, 5], "trim")


@pytest.mark.parametrize("retire_before, survivors", [(at(10), [1, 3, 4, 5]), (0, [1, 2, 3, 4, 5])], ids=["idle-key-gather", "unseen-key-only"])
def test_compact(engine, retire_before, survivors):
    a, b, rows = pair(engine)
    want = np.full(K, SKIP, np.uint64)
    want[survivors] = np.arange(len(survivors), dtype=np.uint64)
    for st in (a, b):
        remap, stats = st.compact(retire_before=retire_before)
        assert np.array_equal(remap, want), remap
        assert st.num_keys == len(survivors) and stats["keys_unseen"] == 1
        assert stats["points_dropped"] == (6 if retire_before else 0)
    sel = np.isin(rows[0], np.asarray(survivors, np.uint64))
    surviving = (want[rows[0][sel].astype(np.int64)], rows[1][sel], rows[2][sel])
    finish(engine, [a, b], surviving, want[[1, 3, 4, 5]], "compact")


def test_merge(engine):
    a, b, rows = pair(engine)
    late = (np.array([3, 5], np.uint64), np.array([at(7), at(22)], np.int64), np.array([1_234_567_890, 2_345_678_901], np.uint64))
    for st in (a, b):
        stats = engine.merge_stream(st, *late, value_op=OP)
        assert (stats["points_inserted"], stats["points_appended"], stats["points_combined"]) == (1, 1, 0), stats
    finish(engine, [a, b], cat(rows, late), [1, 3, 4, 5], "merge")
