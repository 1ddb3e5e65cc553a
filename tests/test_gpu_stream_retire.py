"""GPU, end to end: StreamingAnomalyDetection.retire (TAD_FEATURE_STRING_RETIRE) — the property that matters.  A seeded flow table whose
names churn (every batch introduces pods and services and stops using older ones) is fed to an instance; after retire(idle_before) its
jobs must return exactly the rows of a TWIN instance that was only ever fed the rows whose key survives, survival being decided here on
the host (the key's newest flowEndSeconds >= idle_before).  Then both continue alike — a retired name returns, new ones arrive —, a
snapshot taken after the retire restores to an instance that continues alike too, and the vocabularies hold exactly the strings of the
surviving keys.  Memory: twenty rounds of feed-then-retire with a fixed live set stay bounded while the twin without retire grows."""
import struct

import numpy as np
import pytest

from theia_amd import TadError, _capi as capi
from theia_amd import anomaly_detection as ad
from theia_amd.stream_detection import StreamingAnomalyDetection

pytestmark = pytest.mark.gpu

T0 = 1660202800
STEP = 60
STEPS_PER_BATCH = 6
NAMESPACES = ("shop", "blog", "infra")
MODES = ["svc", "pod"]


def pod(i):
    return NAMESPACES[i % 3], "pod-%d" % i, '{"app":"app%d","gen":"g%d"}' % (i, i // 10)


def svc(i):
    return "ns%d/svc%d:http" % (i % 5, i)


def make_batch(idx, steps, seed, n=400):
    """n flow rows among the pods / services idx (every one of them occurs), at the time steps `steps`"""
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx)
    src, dst, sv = (np.concatenate([idx, rng.choice(idx, n - idx.size)]) for _ in range(3))
    rng.shuffle(dst)
    rng.shuffle(sv)
    step = rng.choice(steps, n)
    value = (1_000_000_000 * (1 + src % 7) + 300_000_000 * (dst % 5) + rng.integers(0, 200_000_000, n)) * np.where(rng.random(n) < 0.04, 40, 1)
    col = lambda who, f: np.array([pod(i)[f] for i in who])
    return {
        "sourcePodNamespace": col(src, 0), "sourcePodName": col(src, 1), "sourcePodLabels": col(src, 2),
        "destinationPodNamespace": col(dst, 0), "destinationPodName": col(dst, 1), "destinationPodLabels": col(dst, 2),
        "destinationIP": np.array(["10.0.0.%d" % (i % 250) for i in dst]), "destinationServicePortName": np.array([svc(i) for i in sv]),
        "flowType": np.ones(n, dtype=np.int64), "flowEndSeconds": (T0 + STEP * step).astype(np.int64),
        "flowStartSeconds": (T0 + STEP * step - 30).astype(np.int64), "throughput": value.astype(np.uint64),
    }


def churn_table():
    """six batches: batch b names the pods / services [10 b, 10 b + 25) at its own six time steps; two later batches bring back the long
    retired 5 and add new ones"""
    first = [make_batch(np.arange(10 * b, 10 * b + 25), np.arange(b * STEPS_PER_BATCH, (b + 1) * STEPS_PER_BATCH), 100 + b) for b in range(6)]
    later = [make_batch(np.concatenate([[5], np.arange(60, 85)]), np.arange(36, 42), 200), make_batch(np.concatenate([[5, 62], np.arange(80, 100)]), np.arange(42, 48), 201)]
    return first, later


IDLE_BEFORE = T0 + STEP * STEPS_PER_BATCH * 4          # a key survives iff batch 4 or 5 named it


def side_keys(flows, mode):
    """per side of the mode: (the rows' key strings as tuples of columns, the column a blank in which drops the row's side in feed)"""
    if mode == "svc":
        return [((flows["destinationServicePortName"],), "destinationServicePortName")]
    return [((flows["destinationPodNamespace"], flows["destinationPodLabels"]), "destinationPodLabels"),
            ((flows["sourcePodNamespace"], flows["sourcePodLabels"]), "sourcePodLabels")]


def survivors_of(batches, mode):
    """per side: {key tuple: newest flowEndSeconds} over all batches -> the set of surviving key tuples"""
    alive = []
    for s in range(len(side_keys(batches[0], mode))):
        newest = {}
        for b in batches:
            cols, _ = side_keys(b, mode)[s]
            for key, t in zip(zip(*[c.tolist() for c in cols]), b["flowEndSeconds"].tolist()):
                newest[key] = max(newest.get(key, t), t)
        alive.append({k for k, t in newest.items() if t >= IDLE_BEFORE})
    return alive


def only_survivors(flows, mode, alive):
    """the batch as the twin gets it: a side whose key does not survive is blanked (feed drops a side with an empty name), a row none of
    whose sides survives is left out"""
    out = {k: v.copy() for k, v in flows.items()}
    any_side = np.zeros(len(flows["flowEndSeconds"]), dtype=bool)
    for (cols, blank), keys in zip(side_keys(flows, mode), alive):
        lives = np.array([k in keys for k in zip(*[c.tolist() for c in cols])])
        out[blank] = np.where(lives, out[blank], "")
        any_side |= lives
    return {k: v[any_side] for k, v in out.items()}


def comparable(rows, mode):
    out = []
    for r in rows:
        r = dict(r)
        if r.get("anomaly") == "NO ANOMALY DETECTED":
            r.pop("flowStartSeconds")
        out.append(tuple((k, struct.pack("<d", v).hex() if isinstance(v, float) else v) for k, v in sorted(r.items())))
    key = lambda t: tuple(str(dict(t).get(c)) for c in ad.KEY_COLUMNS[mode]) + (dict(t)["flowEndSeconds"],)
    return sorted(out, key=lambda t: (key(t), t))


def vocab_strings(inst, i):
    off, data = inst._vocab[i].export()
    raw = data.tobytes()
    return [raw[off[k]:off[k + 1]].decode() for k in range(off.size - 1)]


def same_jobs(a, b, filters=(dict(),), need_anomaly=True):
    for algo in ("EWMA", "DBSCAN"):
        for filt in filters:
            got, want = a.job(algo, "job-1", **filt)[1], b.job(algo, "job-1", **filt)[1]
            assert comparable(got, a.mode) == comparable(want, b.mode), (algo, filt)
            assert not need_anomaly or want[0]["anomaly"] == "true", "no anomalous row: the comparison shows nothing"


FILTERS = {"svc": [dict(svc_port_name=svc(52))], "pod": [dict(pod_label='"APP":"app5'), dict(pod_label='"gen":"g6"', pod_namespace="blog")]}


@pytest.mark.parametrize("mode", MODES)
def test_the_churn_scenario_against_a_twin_fed_only_the_surviving_keys(engine, mode):
    first, later = churn_table()
    alive = survivors_of(first, mode)
    s, t = StreamingAnomalyDetection(engine, mode), StreamingAnomalyDetection(engine, mode)
    r = None
    try:
        for b in first:
            s.feed(b)
            t.feed(only_survivors(b, mode, alive))
        keys_before, values_before, bytes_before = s.num_keys, [v.num_values() for v in s._vocab], s.device_bytes()
        assert s.num_keys > t.num_keys > 0
        out = s.retire(IDLE_BEFORE)
        # what the call says it did
        n_alive = sum(len(a) for a in alive)
        assert (out["keys_before"], out["keys_after"]) == (keys_before, n_alive) and s.num_keys == n_alive == t.num_keys == s.state.num_keys
        assert out["values_before"] == values_before and out["values_after"] == [v.num_values() for v in s._vocab]
        assert out["bytes_before"] == bytes_before and out["bytes_after"] == s.device_bytes() < bytes_before
        # 4. every vocabulary holds exactly the distinct strings of the surviving keys
        for i in range(len(s._vocab)):
            want = {k[i] for a in alive for k in a}
            got = vocab_strings(s, i)
            assert len(got) == len(set(got)) == len(want) and set(got) == want
        assert out["values_after"][-1] < values_before[-1]
        # 3. the jobs are the twin's; 7. the filtered ones too (one of the filters folds case on the device)
        same_jobs(s, t)
        same_jobs(s, t, FILTERS[mode], need_anomaly=False)
        # 6. a snapshot taken after the retire restores to an instance that continues alike
        r = StreamingAnomalyDetection.restore(engine, s.snapshot(), mode)
        same_jobs(r, t)
        # 5. two more batches: a retired name returns (a new string, a new key), new ones arrive
        for b in later:
            for inst in (s, t, r):
                inst.feed(b)
        assert s.num_keys == t.num_keys == r.num_keys
        same_jobs(s, t)
        same_jobs(r, t)
        same_jobs(s, t, FILTERS[mode] + ([dict(svc_port_name=svc(5))] if mode == "svc" else [dict(pod_label='"app":"app5"')]), need_anomaly=False)
    finally:
        for inst in (s, t, r):
            if inst is not None:
                inst.close()


@pytest.mark.parametrize("mode", MODES)
def test_retire_with_nothing_idle_is_a_no_op(engine, mode):
    first, _ = churn_table()
    s = StreamingAnomalyDetection(engine, mode)
    try:
        for b in first[:3]:
            s.feed(b)
        before = s.snapshot()
        nbytes = s.device_bytes()
        out = s.retire(0)                                  # no time rule, and every key has points
        after = s.snapshot()
        assert before.keys() == after.keys()
        for k in before:
            assert before[k].dtype == after[k].dtype and before[k].tobytes() == after[k].tobytes(), k
        assert out["keys_after"] == out["keys_before"] and out["values_after"] == out["values_before"] and out["bytes_after"] == out["bytes_before"] == nbytes
        out = s.retire(T0)                                 # a time before every point
        assert all(before[k].tobytes() == v.tobytes() for k, v in s.snapshot().items()) and out["bytes_after"] == nbytes
    finally:
        s.close()


def test_retire_before_the_first_feed_and_of_everything(engine):
    s = StreamingAnomalyDetection(engine, "svc")
    try:
        out = s.retire(5)
        assert out["keys_before"] == out["keys_after"] == 0 and out["values_after"] == [0]
        first, later = churn_table()
        s.feed(first[0])
        out = s.retire(T0 + STEP * 1000)                   # every key is idle
        assert out["keys_after"] == 0 and out["values_after"] == [0] and s.num_keys == 0 and s.state is None
        assert s.job("EWMA", "j")[1][0]["anomaly"] == "NO ANOMALY DETECTED"
        t = StreamingAnomalyDetection(engine, "svc")
        try:
            for inst in (s, t):
                inst.feed(later[0])
            same_jobs(s, t)
        finally:
            t.close()
    finally:
        s.close()


def test_memory_stays_bounded_over_twenty_rounds_and_grows_without_retire(engine):
    """every round names 40 new pods at its own times and nothing older: with retire the live set is one round's; without, every structure
    keeps every key and string ever met"""
    s, t = StreamingAnomalyDetection(engine, "pod"), StreamingAnomalyDetection(engine, "pod")
    try:
        held, leaked, values = [], [], []
        for rnd in range(20):
            b = make_batch(np.arange(40 * rnd, 40 * rnd + 40), np.arange(4 * rnd, 4 * rnd + 4), 300 + rnd, n=200)
            s.feed(b)
            t.feed(b)
            s.retire(T0 + STEP * 4 * rnd)
            held.append(s.device_bytes())
            leaked.append(t.device_bytes())
            values.append((s._vocab[1].num_values(), t._vocab[1].num_values(), s.num_keys, t.num_keys))
        print("bytes with retire:", held, "\nbytes without:", leaked, "\nvalues / keys:", values[2], values[19])
        assert held[19] <= held[2]
        assert leaked[19] > leaked[2]
        assert values[19][0] == values[2][0] == 40 and values[19][1] == 800 and values[19][2] == values[2][2] and values[19][3] > 10 * values[19][2]
    finally:
        s.close()
        t.close()


def test_a_failure_before_any_vocabulary_moved_leaves_a_consistent_instance(engine, monkeypatch):
    """(simulated: StringDict.compact is patched to raise before it does anything)"""
    first, _ = churn_table()
    alive = survivors_of(first, "svc")
    s, t = StreamingAnomalyDetection(engine, "svc"), StreamingAnomalyDetection(engine, "svc")
    try:
        for b in first:
            s.feed(b)
            t.feed(only_survivors(b, "svc", alive))

        def refuse(*a, **k):
            raise TadError(capi.TAD_ERR_OUT_OF_MEMORY, "no room (dictionary unchanged)")
        monkeypatch.setattr(s._vocab[0], "compact", refuse)
        with pytest.raises(TadError):
            s.retire(IDLE_BEFORE)
        monkeypatch.undo()
        # the keys are retired, the strings are not: consistent, and the next retire finishes the work
        assert s.num_keys == t.num_keys and s._vocab[0].num_values() > t.num_keys
        same_jobs(s, t)
        s.retire(IDLE_BEFORE)
        assert s._vocab[0].num_values() == t.num_keys
        same_jobs(s, t)
    finally:
        s.close()
        t.close()


def test_a_key_dictionary_compaction_that_fails_behind_the_state_poisons_the_instance(engine, monkeypatch):
    """the first of the two pairs that are not atomic: the state is renumbered, the key dictionary still hands out the ids of before.  The
    failure is SIMULATED — KeyDict.compact is patched to raise the library's out-of-memory error after the state's real compaction —
    because no argument makes the real call fail there.  Every later call raises; a snapshot taken before brings the instance back."""
    first, later = churn_table()
    alive = survivors_of(first, "svc")
    s, t = StreamingAnomalyDetection(engine, "svc"), StreamingAnomalyDetection(engine, "svc")
    r = None
    try:
        for b in first:
            s.feed(b)
            t.feed(only_survivors(b, "svc", alive))
        snap = s.snapshot()
        keys = s.num_keys

        def refuse(*a, **k):
            raise TadError(capi.TAD_ERR_OUT_OF_MEMORY, "tad_keydict_compact: out of memory (dictionary unchanged)")
        monkeypatch.setattr(s._dict, "compact", refuse)
        with pytest.raises(TadError):
            s.retire(IDLE_BEFORE)
        monkeypatch.undo()
        assert s.state.num_keys == t.num_keys < keys == s._dict.num_keys()       # the inconsistent pair the docstring names
        for call in (lambda: s.feed(later[0]), lambda: s.job("EWMA", "j"), s.snapshot, s.retire):
            with pytest.raises(RuntimeError) as ei:
                call()
            assert "snapshot" in str(ei.value) and "tad_keydict_compact" in str(ei.value)
        assert s.state.num_keys == t.num_keys and s._dict.num_keys() == keys      # the refused feed touched nothing
        # a failure with nothing to retire is no such case: the dictionary's call is not made, the instance stays usable
        u = StreamingAnomalyDetection.restore(engine, snap, "svc")
        try:
            monkeypatch.setattr(u._dict, "compact", refuse)
            u.retire(0)
            monkeypatch.undo()
            u.feed(later[0])
        finally:
            u.close()
        r = StreamingAnomalyDetection.restore(engine, snap, "svc")
        r.retire(IDLE_BEFORE)
        same_jobs(r, t)
        for b in later:
            r.feed(b)
            t.feed(b)
        same_jobs(r, t)
    finally:
        for inst in (s, t, r):
            if inst is not None:
                inst.close()


def test_a_recode_that_fails_poisons_the_instance_and_a_snapshot_brings_it_back(engine, monkeypatch):
    """the second pair that is not atomic — vocabularies compacted, keys not recoded: every later call raises, and an instance restored
    from a snapshot taken before the retire does the same retire and continues.  The failure inside retire is SIMULATED: KeyDict.recode
    is patched to raise the library's out-of-memory error after the vocabularies were really compacted.  A real refusal cannot be forced
    there — retire's remaps live on the device, so a workspace limit refuses nothing, and the remaps come from the keys' own masks, so
    no value is retired under a key.  What the real call does with a doctored remap is shown at the end, on the lower-level call."""
    first, later = churn_table()
    alive = survivors_of(first, "pod")
    s, t = StreamingAnomalyDetection(engine, "pod"), StreamingAnomalyDetection(engine, "pod")
    r = None
    try:
        for b in first:
            s.feed(b)
            t.feed(only_survivors(b, "pod", alive))
        snap = s.snapshot()

        def refuse(*a, **k):
            raise TadError(capi.TAD_ERR_OUT_OF_MEMORY, "tad_keydict_recode: out of memory (dictionary unchanged)")
        monkeypatch.setattr(s._dict, "recode", refuse)
        with pytest.raises(TadError):
            s.retire(IDLE_BEFORE)
        monkeypatch.undo()
        for call in (lambda: s.feed(later[0]), lambda: s.job("EWMA", "j"), s.snapshot, s.retire):
            with pytest.raises(RuntimeError) as ei:
                call()
            assert "snapshot" in str(ei.value) and "recode" in str(ei.value)
        r = StreamingAnomalyDetection.restore(engine, snap, "pod")
        r.retire(IDLE_BEFORE)
        same_jobs(r, t)
        for b in later:
            r.feed(b)
            t.feed(b)
        same_jobs(r, t)
        # the lower-level call itself refuses a doctored remap and changes nothing: a key still uses the value the remap retires
        cols, side = r._dict.export()
        remap = np.arange(r._vocab[1].num_values(), dtype=np.int64)
        remap[cols[1][0]] = capi.TAD_CODE_NONE
        with pytest.raises(TadError) as ei:
            r._dict.recode({1: remap})
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
        got, _ = r._dict.export()
        assert all(np.array_equal(a, b) for a, b in zip(got, cols))
        same_jobs(r, t)
    finally:
        for inst in (s, t, r):
            if inst is not None:
                inst.close()
