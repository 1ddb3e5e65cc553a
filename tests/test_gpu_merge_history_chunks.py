"""GPU: a combining tad_state_merge on a history state whose keys have 0, 1 and several history chunks.  The merge removes a combined
point's old value from the key's sorted history with k_hist_subtract, one wavefront per chunk of 2048 history values, and its chunk
counts give a key WITHOUT history no chunk (a trim's and a window's give every key one).  The kernel's shortcut "the chunk total equals
the number of keys, so wavefront w is key w" is right only for counts of at least one: with an unused key slot beside a key of two
chunks the total is K too, and the shortcut would leave most of the long key's history unwritten.  So: after the merge every key's
history is its series sorted, the series is the host model's, and the state equals a fresh one streamed over the final points."""
import numpy as np
import pytest
from state_helpers import T_BASE, bits

pytestmark = pytest.mark.gpu

MIN = 60
CHUNK = 2048          # kHistChunk of theia_amd/csrc/tad_internal.h
STATE_FIELDS = ("n", "avg", "m2", "last_t")

# points per key -> the merge's history chunks ceil(len / 2048): the first and the last layout sum to K with a key of two chunks
LAYOUTS = {"empty + long": (0, 3000), "short + long": (5, 3000), "long, two empty, long": (3000, 0, 0, 2500),
           "empty, three chunks, short": (0, 4500, 7)}


def points(lens, seed):
    """(key, time, value) of every key's points, minute lattice from T_BASE, in (key, time) order"""
    rng = np.random.default_rng(seed)
    k = np.repeat(np.arange(len(lens), dtype=np.uint64), lens)
    t = np.concatenate([T_BASE + MIN * np.arange(n, dtype=np.int64) for n in lens])
    v = rng.integers(1_000_000, 2_000_000_000, size=k.size).astype(np.uint64)
    return k, t, v


def segments(ln, vals):
    o = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
    return [vals[o[i]:o[i + 1]] for i in range(ln.size)]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_combining_merge_keeps_history_equal_to_the_sorted_series(engine, name):
    lens = LAYOUTS[name]
    K = len(lens)
    chunks = [(n + CHUNK - 1) // CHUNK for n in lens]
    print(name, "history chunks per key", chunks, "total", sum(chunks), "keys", K)
    if name in ("empty + long", "long, two empty, long"):
        assert sum(chunks) == K and max(chunks) > 1 and min(chunks) == 0       # the layout the shortcut must not be taken on
    k, t, v = points(lens, seed=len(name))
    st = engine.state_create(K, history=True, series=True, times=True)
    engine.run_stream(st, k, t, v, value_op="max")
    hl, hv = st.export_history()
    assert np.array_equal(hl, np.array(lens, np.uint64))
    # one re-sent point of every non-empty key, in its newest third, with a larger value: combined under max, the old value leaves the history
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    idx = np.array([first[i] + (2 * lens[i]) // 3 for i in range(K) if lens[i]], np.int64)
    nv = v[idx] + np.uint64(12345)
    stats = engine.merge_stream(st, k[idx], t[idx], nv, value_op="max")
    assert stats["points_combined"] == idx.size and stats["points_inserted"] == 0 and stats["points_appended"] == 0, stats
    want = v.copy()
    want[idx] = nv
    sl, sv = st.export_series()
    hl, hv = st.export_history()
    assert np.array_equal(sl, np.array(lens, np.uint64)) and np.array_equal(hl, sl)
    assert np.array_equal(sv, want) and np.array_equal(st.export_times(), t)
    for key, (s, h) in enumerate(zip(segments(sl, sv), segments(hl, hv))):
        diff = int((np.sort(s) != h).sum())
        assert diff == 0, (name, key, "history values that differ from the sorted series", diff, "of", h.size)
    fresh = engine.state_create(K, history=True, series=True, times=True)
    engine.run_stream(fresh, k, t, want, value_op="max")
    a, b = st.export(), fresh.export()
    for f in STATE_FIELDS:
        assert np.array_equal(bits(a[f]), bits(b[f])), (name, f)
    # what reads the history next: DBSCAN's verdicts from the state are the batch job's over the final points
    got = engine.run_state(st, algo="DBSCAN", emit_all=True)
    ref = engine.run("DBSCAN", k, t, want, K, value_op="max", emit_all=True)
    for f in ("key_id", "flow_end_s", "throughput", "algo_calc", "stddev", "anomaly"):
        assert np.array_equal(bits(np.asarray(got[f])), bits(np.asarray(ref[f]))), (name, f)
    fresh.close()
    st.close()
