"""GPU: the persistent key dictionary (tad_keydict, include/tad.h) — key tuples -> dense ids that stay the same from batch to batch, new
ids in order of first appearance.  The oracle is a Python dict over the kept virtual rows of every batch in sequential order
([side a ++ side b] per batch); one-sided cases are also held against tad_factorize and the pandas factorisation of the concatenation
of the batches, restricted to each batch.  Every dictionary starts at the smallest table (expected_keys=1) unless a case says otherwise,
so the growth of the table and of the key records is on the path of nearly every case."""
import ctypes as C

import numpy as np
import pytest

from oracle import tad_oracle as orc
from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import SKIP, assert_keydict_unchanged, host, keydict_snapshot, pandas_ids
from state_helpers import ROW_FIELDS, U64, bits

pytestmark = pytest.mark.gpu


class DictOracle:
    """tuple (side, columns...) -> id, ids in order of first appearance over the kept virtual rows [side a ++ side b] of every batch"""

    def __init__(self):
        self.ids = {}

    def run(self, cols, keep=None, cols_b=None, keep_b=None, insert=True):
        n = len(cols[0])
        before = len(self.ids)
        out, first = [], []
        for side, (cs, kp) in enumerate(((cols, keep), (cols_b, keep_b))):
            if cs is None:
                out.append(None)
                continue
            k = np.full(n, SKIP, dtype=U64)
            rows = list(zip(*[np.asarray(c).tolist() for c in cs]))
            for i in (range(n) if kp is None else np.flatnonzero(kp).tolist()):
                t = (side,) + rows[i]
                j = self.ids.get(t)
                if j is None:
                    if not insert:
                        continue
                    j = len(self.ids)
                    self.ids[t] = j
                    first.append(i + side * n)
                k[i] = j
            out.append(k)
        return out[0], out[1], np.array(first, dtype=U64), before

    def tuples(self):
        """(columns, side) of key 0 .. K - 1"""
        ts = sorted(self.ids, key=self.ids.get)
        ncols = len(ts[0]) - 1 if ts else 0
        return [np.array([t[c + 1] for t in ts], dtype=np.int64) for c in range(ncols)], np.array([t[0] for t in ts], dtype=np.uint8)


def dev(engine, cols):
    return None if cols is None else [DeviceArray.from_host(engine, np.ascontiguousarray(c)) for c in cols]


def assert_batch(got, want, what=""):
    k1, k2, fr, before = got
    w1, w2, wfr, wbefore = want
    assert before == wbefore, (what, before, wbefore)
    assert np.array_equal(host(k1), w1), what
    assert (k2 is None) == (w2 is None) and (w2 is None or np.array_equal(host(k2), w2)), what
    assert np.array_equal(host(fr), wfr), what


def random_columns(rng, ncols, n, card):
    """test_gpu_factorize's tuples: negative and large values"""
    span = np.array([card, 7, 3, 5, 2, 4, 2, 3][:ncols])
    return [(rng.integers(0, span[c], size=n) * (1 if c % 2 == 0 else -977) + (c << 40)).astype(np.int64) for c in range(ncols)]


def cut(n, parts):
    """batch bounds: 1 batch, 2 unequal ones, or 7 of unequal size with an empty one and a 1-row one"""
    if parts == 1:
        return [(0, n)]
    if parts == 2:
        return [(0, n // 3), (n // 3, n)]
    e = [0, n // 20, n // 20, n // 20 + 1, n // 3, n // 3 + n // 100, (7 * n) // 10, n]
    return list(zip(e[:-1], e[1:]))


# ---- 1. one-sided batches == tad_factorize on the concatenation ----
@pytest.mark.parametrize("ncols,n,card", [(1, 100_000, 500), (3, 200_000, 40), (6, 150_000, 12), (8, 50_000, 5), (2, 300_000, 100_000)])
def test_batches_equal_factorize_on_the_concatenation(engine, ncols, n, card):
    rng = np.random.default_rng(ncols * 1000 + n)
    cols = random_columns(rng, ncols, n, card)
    keep = rng.random(n) < 0.8
    fz_ids, _, fz_first = engine.factorize(cols, keep)            # ONE call on the concatenation
    pd_ids, pd_first = pandas_ids(cols, keep)
    assert np.array_equal(fz_ids, pd_ids[0]) and np.array_equal(fz_first, pd_first)
    for parts in (1, 2, 7):
        oracle = DictOracle()
        dh, dd = engine.key_dict(ncols, 1), engine.key_dict(ncols, 1)
        for lo, hi in cut(n, parts):
            bc, bk = [c[lo:hi] for c in cols], keep[lo:hi]
            want = oracle.run(bc, bk)
            got_h = dh.encode(bc, bk)
            got_d = dd.encode(dev(engine, bc), bk)
            assert isinstance(got_d[0], DeviceArray) and isinstance(got_h[0], np.ndarray)      # results live where the inputs live
            assert_batch(got_h, want, (parts, lo, hi, "host"))
            assert_batch(got_d, want, (parts, lo, hi, "device"))
            assert np.array_equal(got_h[0], fz_ids[lo:hi]), (parts, lo, hi)                     # tad_factorize of the concatenation, this batch's rows
            new = (fz_first >= lo) & (fz_first < hi)                                            # the keys whose first row lies in this batch
            assert np.array_equal(got_h[2], fz_first[new] - U64(lo)), (parts, lo, hi)
            assert dh.num_keys() == dd.num_keys() == len(oracle.ids) == want[3] + int(new.sum())
        assert dh.num_keys() == fz_first.size
        dh.close(), dd.close()


# ---- 2. two sides: the side is part of the tuple, the order is b1.a, b1.b, b2.a, b2.b ----
def test_two_sided_batches_in_sequential_order(engine):
    rng = np.random.default_rng(21)
    oracle = DictOracle()
    dh, dd = engine.key_dict(3, 1), engine.key_dict(3, 1)
    for b, n in enumerate((30_000, 1, 50_000, 20_000)):
        ca, cb = random_columns(rng, 3, n, 300 * (b + 1)), random_columns(rng, 3, n, 200 * (b + 1))
        ka, kb = rng.random(n) < 0.8, rng.random(n) < 0.5
        if b == 3:                    # a one-sided batch after two-sided ones
            cb = kb = None
        want = oracle.run(ca, ka, cb, kb)
        assert_batch(dh.encode(ca, ka, cb, kb), want, (b, "host"))
        assert_batch(dd.encode(dev(engine, ca), ka, dev(engine, cb), kb), want, (b, "device"))
    assert dh.num_keys() == dd.num_keys() == len(oracle.ids)
    cols, side = dh.export()
    wc, ws = oracle.tuples()
    assert np.array_equal(side, ws) and all(np.array_equal(a, b) for a, b in zip(cols, wc))
    dh.close(), dd.close()


def test_the_side_is_part_of_the_tuple(engine):
    d = engine.key_dict(2, 1)
    t = [np.array([5, 6], np.int64), np.array([-1, -2], np.int64)]              # tuples X = (5, -1), Y = (6, -2)
    other = [np.array([9, 9], np.int64), np.array([9, 9], np.int64)]            # Z = (9, 9) twice
    k1, k2, fr, before = d.encode(other, None, t, None)                         # batch 1: a = Z, Z; b = X, Y
    assert before == 0 and k1.tolist() == [0, 0] and k2.tolist() == [1, 2] and fr.tolist() == [0, 2, 3]
    k1, k2, fr, before = d.encode(other, None, [c[::-1].copy() for c in t], None)   # batch 2: b = Y, X — first seen on side b, same ids
    assert before == 3 and k1.tolist() == [0, 0] and k2.tolist() == [2, 1] and fr.size == 0
    k1, k2, fr, before = d.encode(t, None, other, None)                         # the same columns on side a (and Z on side b): other ids
    assert before == 3 and k1.tolist() == [3, 4] and k2.tolist() == [5, 5] and fr.tolist() == [0, 1, 2]
    k1, k2, fr, before = d.encode(t)                                            # a one-sided batch is side a
    assert before == 6 and k2 is None and k1.tolist() == [3, 4] and fr.size == 0
    cols, side = d.export()
    assert side.tolist() == [0, 1, 1, 0, 0, 1] and cols[0].tolist() == [9, 5, 6, 5, 6, 9] and cols[1].tolist() == [9, -1, -2, -1, -2, 9]
    d.close()


# ---- 3. wavefront corners ----
def test_one_tuple_on_every_lane_new_then_known(engine):
    same = np.full(70_000, -5, dtype=np.int64)
    d = engine.key_dict(2, 1)
    k1, _, fr, before = d.encode([same, same])                                  # every lane of every wavefront misses on the same tuple
    assert before == 0 and (k1 == 0).all() and fr.tolist() == [0] and d.num_keys() == 1
    k1, _, fr, before = d.encode([same, same])                                  # ... and hits on it
    assert before == 1 and (k1 == 0).all() and fr.size == 0 and d.num_keys() == 1
    d.close()


def test_known_and_new_tuples_alternate_row_by_row(engine):
    d, oracle = engine.key_dict(2, 1), DictOracle()
    known = [np.arange(3000, dtype=np.int64), np.arange(3000, dtype=np.int64) * -3]
    assert_batch(d.encode(known), oracle.run(known))
    n = 40_000
    a = np.where(np.arange(n) % 2 == 0, np.arange(n) % 3000, 10_000 + np.arange(n) // 4).astype(np.int64)     # odd rows: new tuples, each twice
    mixed = [a, a * -3]
    want = oracle.run(mixed)
    assert want[2].size == n // 4
    assert_batch(d.encode(dev(engine, mixed)), want)
    assert d.num_keys() == 3000 + n // 4
    d.close()


def test_growth_within_and_between_calls_keeps_every_id(engine):
    rng = np.random.default_rng(5)
    vals = rng.permutation(1 << 20)[:40_000].astype(np.int64) - (1 << 19)
    cols = [vals, vals * 1_000_003]                                             # 40 000 distinct tuples
    d, oracle = engine.key_dict(2, 1), DictOracle()
    small = d.nbytes()
    seen, sizes = [], [small]
    for lo, hi in ((0, 20_000), (20_000, 20_100), (20_100, 33_000), (33_000, 40_000)):
        bc = [c[lo:hi] for c in cols]
        want = oracle.run(bc)
        assert_batch(d.encode(bc), want, (lo, hi))
        assert np.array_equal(want[0], np.arange(lo, hi, dtype=U64)) and d.num_keys() == hi
        seen.append((bc, want[0]))
        sizes.append(d.nbytes())
        for old, ids in seen:                                                   # every earlier batch, after this call's growth
            k1, _ = d.lookup(old)
            assert np.array_equal(k1, ids), (lo, hi)
    assert sizes[1] >= 16 * 20_000 and sizes[-1] > sizes[1] > small              # the table (>= 2 slots per key) and the records grew
    ec, es = d.export()
    assert np.array_equal(ec[0], cols[0]) and np.array_equal(ec[1], cols[1]) and not es.any()
    d.close()


def test_tuples_that_differ_only_in_the_last_of_eight_columns(engine):
    n = 5000
    base = [np.full(n, (c + 1) * -(1 << 50), dtype=np.int64) for c in range(7)]
    last = (np.arange(n) % 1250).astype(np.int64)
    d, oracle = engine.key_dict(8, 1), DictOracle()
    want = oracle.run(base + [last])
    assert want[2].size == 1250
    assert_batch(d.encode(base + [last]), want)
    assert_batch(d.encode(dev(engine, base + [last + 1000])), oracle.run(base + [last + 1000]))      # 250 known, 1000 new
    assert d.num_keys() == 2250
    d.close()


def test_nothing_kept_and_an_empty_batch(engine):
    d = engine.key_dict(1, 1)
    k1, _, fr, before = d.encode([np.zeros(1000, np.int64)], np.zeros(1000, bool))
    assert before == 0 and (k1 == SKIP).all() and fr.size == 0 and d.num_keys() == 0
    k1, _, fr, before = d.encode([np.zeros(0, np.int64)])
    assert before == 0 and k1.size == 0 and fr.size == 0
    k1, k2, fr, before = d.encode([np.arange(4, dtype=np.int64)], np.array([0, 1, 0, 1], bool), [np.arange(4, dtype=np.int64)], np.zeros(4, bool))
    assert before == 0 and k1.tolist() == [int(SKIP), 0, int(SKIP), 1] and (k2 == SKIP).all() and fr.tolist() == [1, 3]
    d.close()


def test_new_first_row_cap_caps_the_list_never_the_ids(engine):
    d = engine.key_dict(1, 1)
    alld = np.arange(6000, dtype=np.int64)[::-1].copy()
    k1, _, fr, before = d.encode([alld], max_new=10)
    assert fr.tolist() == list(range(10)) and np.array_equal(k1, np.arange(6000, dtype=U64)) and d.num_keys() == 6000
    k1, _, fr, before = d.encode(dev(engine, [alld + 3000]), max_new=10)
    assert before == 6000 and fr.to_host().tolist() == list(range(10)) and int(k1.to_host().max()) == 8999 and d.num_keys() == 9000
    d.close()


# ---- 4. lookup: read-only ----
def test_lookup_is_read_only(engine):
    rng = np.random.default_rng(8)
    d, oracle = engine.key_dict(3, 1), DictOracle()
    cols = random_columns(rng, 3, 20_000, 900)
    assert_batch(d.encode(cols), oracle.run(cols))
    snap = keydict_snapshot(d)
    size = d.nbytes()
    probe = random_columns(rng, 3, 30_000, 2500)                                # about a third of these tuples are known
    keep = rng.random(30_000) < 0.7
    want = oracle.run(probe, keep, probe, None, insert=False)
    unknown = int((want[0][keep] == SKIP).sum())
    assert 0 < unknown < int(keep.sum()) and (want[1] == SKIP).all()             # side b never saw a tuple
    k1, k2 = d.lookup(probe, keep, probe, None)
    assert np.array_equal(k1, want[0]) and np.array_equal(k2, want[1])
    k1, k2 = d.lookup(dev(engine, probe), keep)
    assert np.array_equal(k1.to_host(), want[0]) and k2 is None
    assert_keydict_unchanged(d, snap)
    assert d.nbytes() == size
    d.close()


# ---- 5. export / import ----
def test_export_in_slices_and_import_continues_with_the_same_ids(engine):
    rng = np.random.default_rng(13)
    d, oracle = engine.key_dict(4, 1), DictOracle()
    batches = [(random_columns(rng, 4, 8000, 400 * (b + 1)), random_columns(rng, 4, 8000, 150)) for b in range(4)]
    for ca, cb in batches[:2]:
        assert_batch(d.encode(ca, None, cb, None), oracle.run(ca, None, cb, None))
    K = d.num_keys()
    wc, ws = oracle.tuples()
    cols, side = d.export()
    assert K == len(oracle.ids) and np.array_equal(side, ws) and all(np.array_equal(a, b) for a, b in zip(cols, wc))
    for first, cnt in ((0, 1), (1, K // 2), (1 + K // 2, K - 1 - K // 2), (K, 0)):          # slices, first_key > 0
        sc, ss = d.export(first, cnt)
        assert np.array_equal(ss, ws[first:first + cnt]) and all(np.array_equal(a, b[first:first + cnt]) for a, b in zip(sc, wc))
    with pytest.raises(TadError):
        d.export(K - 1, 2)
    fresh = engine.key_dict(4, 1)
    fresh.load(cols, side)
    assert fresh.num_keys() == K
    for ca, cb in batches[2:]:                                                   # the original and the restored one continue alike
        want = oracle.run(ca, None, cb, None)
        assert_batch(d.encode(ca, None, cb, None), want)
        assert_batch(fresh.encode(dev(engine, ca), None, dev(engine, cb), None), want)
    a, b = keydict_snapshot(d), keydict_snapshot(fresh)
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    d.close(), fresh.close()


def test_import_refusals_leave_the_dictionary_unchanged(engine):
    d = engine.key_dict(2, 1)
    cols = [np.arange(5000, dtype=np.int64), np.arange(5000, dtype=np.int64) % 7]
    dup = [c.copy() for c in cols]
    dup[0][4321], dup[1][4321] = dup[0][17], dup[1][17]                          # one duplicate tuple among 5000
    for bad_cols, bad_side in ((dup, None), (cols, np.where(np.arange(5000) == 99, 2, 0).astype(np.uint8))):
        with pytest.raises(TadError) as ei:
            d.load(bad_cols, bad_side)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and d.num_keys() == 0
    side = (np.arange(5000) % 2).astype(np.uint8)
    d.load(dup, np.where(np.arange(5000) == 4321, 1, 0).astype(np.uint8))        # the same columns on the other side: another tuple
    assert d.num_keys() == 5000
    snap = keydict_snapshot(d)
    with pytest.raises(TadError) as ei:                                          # a dictionary that holds keys
        d.load(cols, side)
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
    assert_keydict_unchanged(d, snap)
    k1, _, fr, before = d.encode([dup[0][:20], dup[1][:20]])                     # the imported keys are found
    assert before == 5000 and k1.tolist() == list(range(20)) and fr.size == 0
    d.close()


# ---- 6. refusals leave the dictionary unchanged ----
def raw_encode(engine, d, n_cols, cols_a, cols_b, n):
    arr_a = (C.c_void_p * len(cols_a))(*[None if c is None else c.ctypes.data for c in cols_a])
    arr_b = (C.c_void_p * len(cols_b))(*[None if c is None else c.ctypes.data for c in cols_b]) if cols_b is not None else None
    kc = capi.KeyColumns(n_rows=n, n_cols=n_cols, cols_a=arr_a, keep_a=None, cols_b=arr_b, keep_b=None, memory=capi.TAD_MEM_HOST)
    k1, k2, fr = np.zeros(n, U64), np.zeros(n, U64), np.zeros(2 * n, U64)
    before, after = capi.u64(), capi.u64()
    return engine._lib.tad_keydict_encode(engine._h, d._h, C.byref(kc), k1.ctypes.data, k2.ctypes.data, fr.ctypes.data, 2 * n, C.byref(before), C.byref(after))


def test_bad_arguments_leave_the_dictionary_unchanged(engine):
    d = engine.key_dict(3, 1)
    c = [np.arange(100, dtype=np.int64) + 1000 * i for i in range(3)]
    d.encode(c)
    snap = keydict_snapshot(d)
    new = [x + 500 for x in c]
    assert raw_encode(engine, d, 2, new[:2], None, 100) == capi.TAD_ERR_INVALID_ARGUMENT        # n_cols is not the dictionary's
    assert raw_encode(engine, d, 4, new + [new[0]], None, 100) == capi.TAD_ERR_INVALID_ARGUMENT
    assert raw_encode(engine, d, 3, [new[0], None, new[2]], None, 100) == capi.TAD_ERR_INVALID_ARGUMENT      # a NULL column
    assert raw_encode(engine, d, 3, new, [new[0], new[1], None], 100) == capi.TAD_ERR_INVALID_ARGUMENT      # side b is a column short
    for args in ((new[:2],), (new, None, new[:2], None)):
        with pytest.raises(TadError) as ei:
            d.encode(*args)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
        with pytest.raises(TadError):
            d.lookup(*args)
    assert_keydict_unchanged(d, snap)
    assert raw_encode(engine, d, 3, new, None, 100) == capi.TAD_OK and d.num_keys() == 200      # the same batch, passed properly
    d.close()


def test_workspace_limit_refuses_a_big_batch_and_leaves_the_dictionary_unchanged(engine):
    """Scratch (include/tad.h): V bytes of miss flags; a batch with unknown tuples adds 8 V bytes of local ids, 8 bytes per miss row and
    tad_factorize's scratch, whose table alone is 8 bytes x (the power of two >= 2 V).  With a limit of 1 MiB a device batch of 1000 rows
    needs about 50 KB and passes; one of 100 000 unknown tuples needs more than 16 x 100 000 bytes for that table and is refused with
    tad_factorize's own code — after the probe, before the dictionary is touched.  The same 100 000 rows with KNOWN tuples need the
    flags only, and pass."""
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    try:
        d = small.key_dict(2, 1)
        first = [np.arange(1000, dtype=np.int64), np.arange(1000, dtype=np.int64) * -7]
        k1, _, fr, before = d.encode(dev(small, first))
        assert before == 0 and np.array_equal(k1.to_host(), np.arange(1000, dtype=U64)) and d.num_keys() == 1000
        snap = keydict_snapshot(d)
        big = [np.arange(100_000, dtype=np.int64) + 5000, np.arange(100_000, dtype=np.int64)]
        with pytest.raises(TadError) as ei:
            d.encode(dev(small, big))
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        with pytest.raises(TadError) as ei:
            small.factorize(dev(small, big))                                     # the existing call refuses the same batch the same way
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        assert_keydict_unchanged(d, snap)
        known = [np.arange(100_000, dtype=np.int64) % 1000, (np.arange(100_000, dtype=np.int64) % 1000) * -7]
        k1, _, fr, before = d.encode(dev(small, known))
        assert before == 1000 and fr.n == 0 and np.array_equal(k1.to_host(), np.arange(100_000, dtype=U64) % U64(1000))
        assert_keydict_unchanged(d, snap)
        d.close()
    finally:
        small.close()


# ---- 7. end to end: stream the batches through the dictionary into a state, ask the state for the window's verdicts ----


def test_streaming_ingest_through_the_dictionary_equals_the_batch_job(engine):
    """A second-resolution table of 60 000 rows whose ~3000 six-column keys appear over time, in ARRIVAL order with a few late rows, cut
    into 6 batches.  Per batch: encode -> tad_state_resize when num_keys grew -> tad_state_merge.  tad_run_state then returns exactly
    the rows of tad_run over the whole table with the ids of ONE tad_factorize call."""
    rng = np.random.default_rng(77)
    n, nkeys, span = 60_000, 3000, 7200
    pos = np.arange(n)
    reach = 40 + (nkeys - 40) * pos // n                                         # the keys a row can carry grow with time
    kidx = (rng.random(n) * reach).astype(np.int64)
    t = orc.SYNTH_T_BASE + pos * span // n + rng.integers(0, 3, size=n)
    late = rng.random(n) < 0.01                                                  # a few rows arrive up to ten minutes late
    t = np.where(late, np.maximum(t - rng.integers(60, 600, size=n), orc.SYNTH_T_BASE), t).astype(np.int64)
    v = rng.integers(1, 1 << 30, size=n).astype(np.uint64)
    v[rng.random(n) < 0.002] += np.uint64(1 << 36)
    cols = [kidx % 13, (kidx % 7) * -977, kidx // 91, kidx % 3 + (1 << 40), kidx % 2, kidx * 31 % 5]       # (kidx -> tuple is injective: 13 x 7 x kidx // 91)
    cols = [c.astype(np.int64) for c in cols]
    key_all, _, first_all = engine.factorize(cols)                               # ONE call over the whole table
    K = first_all.size
    assert 2500 < K <= nkeys
    d = engine.key_dict(6, 1)
    st = engine.state_create(1, history=True, series=True, times=True)
    edges = [0, 4000, 15_000, 15_001, 31_000, 47_000, n]
    for lo, hi in zip(edges[:-1], edges[1:]):
        ids, _, fr, before = d.encode([c[lo:hi] for c in cols])
        assert np.array_equal(ids, key_all[lo:hi])
        if d.num_keys() > st.num_keys:
            st.resize(d.num_keys())
        engine.merge_stream(st, ids, t[lo:hi], v[lo:hi], value_op="sum")
    assert d.num_keys() == st.num_keys == K
    for algo in ("EWMA", "DBSCAN"):
        for emit_all in (False, True):
            got = engine.run_state(st, algo=algo, emit_all=emit_all)
            want = engine.run(algo, key_all, t, v, K, value_op="sum", emit_all=emit_all)
            assert got.n_rows == want.n_rows > 0, (algo, emit_all)
            for f in ROW_FIELDS:
                assert np.array_equal(bits(np.asarray(got[f])), bits(np.asarray(want[f]))), (algo, emit_all, f)
    st.close(), d.close()
