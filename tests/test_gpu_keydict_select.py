"""GPU: a key mask from the dictionary's tuples (tad_keydict_select, include/tad.h).  keep[k] = 1 iff key k's side is the wanted one and
every term's mask byte at the key's code is not 0 — tad_mask_rows' rule on the dictionary's records.  The reference is numpy on
KeyDict.export(): the tuples and sides the dictionary itself reports.  Shapes: every record width (16 .. 80 bytes), key counts around one
workgroup (256) and several, dictionaries that grew, were compacted, hold two sides; masks and output in host memory, in device memory
and at device addresses offset by 1 and 3 bytes."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import assert_keydict_unchanged, keydict_snapshot

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 7, 8)
KEY_COUNTS = (0, 1, 255, 256, 257, 1025)
CARD = (23, 7, 5, 3, 11, 4, 6, 9)          # codes per column: column c holds values in [0, CARD[c])


def space(ncols, K):
    """(M, rest): tuple j < M has the mixed-radix digits of j in columns 1 .. ncols - 1 (CARD) and the quotient in column 0"""
    rest = int(np.prod(CARD[1:ncols], dtype=np.int64))
    return max(K, CARD[0] * rest), rest


def card_of(ncols, K, c):
    """codes of column c: CARD[c], column 0 as many as K distinct tuples need (at least CARD[0])"""
    M, rest = space(ncols, K)
    return -(-M // rest) if c == 0 else CARD[c]


def tuples(ncols, K, seed=0):
    """K distinct tuples of ncols code columns in a seeded order, column c in [0, card_of(ncols, K, c))"""
    rng = np.random.default_rng(1000 * ncols + K + seed)
    M, rest = space(ncols, K)
    if M <= 8 * K + 64:
        j = rng.permutation(M)[:K]
    else:
        draw = rng.integers(0, M, size=2 * K + 64)
        _, first = np.unique(draw, return_index=True)
        j = draw[np.sort(first)][:K]
    assert j.size == K
    cols = [None] * ncols
    q = j.astype(np.int64)
    for c in range(ncols - 1, 0, -1):
        cols[c] = q % CARD[c]
        q = q // CARD[c]
    cols[0] = q
    return cols


def filled(engine, ncols, K, two_sided=False, expected_keys=1, seed=0):
    d = engine.key_dict(ncols, expected_keys=expected_keys)
    cols = tuples(ncols, K, seed)
    if K:
        if two_sided:                                         # the same tuples on both sides: 2 K keys, side a first
            d.encode(cols, cols_b=cols)
        else:
            d.encode(cols)
    assert d.num_keys() == K * (2 if two_sided else 1)
    return d


def reference(d, terms, side=None):
    cols, sd = d.export()
    keep = np.ones(sd.size, bool)
    if side is not None:
        keep &= sd == side
    for c, m in terms:
        keep &= np.asarray(m)[cols[c]] != 0
    return keep.astype(np.uint8)


def host_of(keep):
    return keep.to_host() if isinstance(keep, DeviceArray) else np.asarray(keep)


def term_sets(ncols, K, rng):
    """name -> terms: none; one; two on different columns; two on the same column; eight; only the last code; mask bytes 2 and 255"""
    def mask(c, p=0.5):
        return (rng.random(card_of(ncols, K, c)) < p).astype(np.uint8)
    last = np.zeros(card_of(ncols, K, 0), np.uint8)
    last[-1] = 1
    odd = mask(0)
    odd = np.where(odd != 0, np.where(np.arange(odd.size) % 2 == 0, 2, 255), 0).astype(np.uint8)
    sets = {"none": [], "one": [(0, mask(0))], "same column twice": [(0, mask(0, 0.7)), (0, mask(0, 0.7))],
            "eight": [(t % ncols, mask(t % ncols, 0.85)) for t in range(8)], "last code only": [(0, last)], "bytes 2 and 255": [(0, odd)]}
    if ncols > 1:
        sets["two columns"] = [(0, mask(0)), (ncols - 1, mask(ncols - 1))]
    return sets


# ---- 1. every record width, key count and term set, in host and in device memory ----
@pytest.mark.parametrize("K", KEY_COUNTS)
@pytest.mark.parametrize("ncols", WIDTHS)
def test_select_equals_numpy_on_the_exported_tuples(engine, ncols, K):
    d = filled(engine, ncols, K)
    snap = keydict_snapshot(d)
    rng = np.random.default_rng(ncols * 7919 + K)
    some = 0
    for name, terms in term_sets(ncols, K, rng).items():
        want = reference(d, terms)
        for out in ("host", "device"):
            keep, n_sel = d.select(terms, out=out)
            got = host_of(keep)
            assert got.dtype == np.uint8 and got.size == K, (name, out)
            assert np.array_equal(got, want), (name, out, ncols, K)
            assert n_sel == int(want.sum()), (name, out, n_sel, int(want.sum()))
        some += int(0 < want.sum() < K)
        if name == "none":
            assert want.all()
    if K >= 255:
        assert some >= 4, some                               # mixed masks: the comparisons are not vacuous
    assert_keydict_unchanged(d, snap)
    d.close()


# ---- 2. sides ----
@pytest.mark.parametrize("ncols,K", [(1, 257), (3, 513), (8, 300)])
def test_side_selects_on_a_two_sided_dictionary(engine, ncols, K):
    d = filled(engine, ncols, K, two_sided=True)
    _, sd = d.export()
    assert (sd == 0).sum() == K and (sd == 1).sum() == K
    rng = np.random.default_rng(K)
    m = (rng.random(card_of(ncols, K, 0)) < 0.5).astype(np.uint8)
    for side in (None, -1, 0, 1):
        for terms in ([], [(0, m)]):
            want = reference(d, terms, None if side in (None, -1) else side)
            keep, n_sel = d.select(terms, side=side, out="host")
            assert np.array_equal(keep, want) and n_sel == int(want.sum()), (side, len(terms))
            if side in (0, 1) and not terms:
                assert n_sel == K and np.array_equal(keep, (sd == side).astype(np.uint8))
    d.close()


# ---- 3. after growth and after compact ----
def test_after_the_table_and_the_records_grew_twice(engine):
    d = engine.key_dict(2, expected_keys=1)
    before = d.nbytes()
    cols = tuples(2, 160)
    sizes = []
    for lo, hi in ((0, 20), (20, 70), (70, 160)):             # 20, 70, 160 keys: the smallest table (64 slots, 32 records) grows at 33 and at 65
        d.encode([c[lo:hi] for c in cols])
        sizes.append(d.nbytes())
    assert before < sizes[1] < sizes[2], (before, sizes)
    m0 = (np.arange(card_of(2, 160, 0)) % 3 != 0).astype(np.uint8)
    m1 = (np.arange(CARD[1]) % 2 == 0).astype(np.uint8)
    want = reference(d, [(0, m0), (1, m1)])
    assert 0 < want.sum() < 160
    for out in ("host", "device"):
        keep, n_sel = d.select([(0, m0), (1, m1)], out=out)
        assert np.array_equal(host_of(keep), want) and n_sel == int(want.sum())
    d.close()


def test_after_compact(engine):
    K = 600
    d = filled(engine, 3, K)
    remap = np.full(K, capi.TAD_KEY_SKIP, np.uint64)
    live = np.flatnonzero(np.arange(K) % 3 != 1)
    remap[live] = np.arange(live.size, dtype=np.uint64)
    assert d.compact(remap) == live.size
    m = (np.arange(card_of(3, K, 0)) % 2 == 0).astype(np.uint8)
    want = reference(d, [(0, m)])
    assert want.size == live.size and 0 < want.sum() < live.size
    keep, n_sel = d.select([(0, m)], out="host")
    assert np.array_equal(keep, want) and n_sel == int(want.sum())
    with pytest.raises(TadError) as ei:                       # a mask sized for the dictionary before the compact is stale
        raw_select(engine, d, [(0, m)], np.zeros(K, np.uint8))
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
    d.close()


# ---- 4. device addresses that are not aligned ----
def raw_select(engine, d, terms, keep, side=-1, memory=capi.TAD_MEM_HOST, keep_len=None, n_terms=None, mask_ptrs=None, mask_lens=None, cols=None):
    """the C call itself; keep: a numpy array (host) or a device address"""
    nt = len(terms) if n_terms is None else n_terms
    arrs = [np.ascontiguousarray(m, dtype=np.uint8) for _, m in terms]
    ptrs = mask_ptrs if mask_ptrs is not None else [a.ctypes.data for a in arrs]
    lens = mask_lens if mask_lens is not None else [a.size for a in arrs]
    cs = cols if cols is not None else [c for c, _ in terms]
    n = max(len(ptrs), 1)
    kp = keep.ctypes.data if isinstance(keep, np.ndarray) else keep
    kl = (keep.size if isinstance(keep, np.ndarray) else 0) if keep_len is None else keep_len
    n_sel = capi.u64(12345)
    rc = engine._lib.tad_keydict_select(engine._h, d._h, nt, (capi.i32 * n)(*cs), (C.c_void_p * n)(*ptrs), (capi.u64 * n)(*lens), side, kp, kl, memory,
                                        C.byref(n_sel))
    engine._check(rc)
    return int(n_sel.value)


@pytest.mark.parametrize("shift", (1, 3))
def test_device_masks_and_output_at_odd_addresses(engine, shift):
    K = 1025
    d = filled(engine, 3, K)
    rng = np.random.default_rng(shift)
    m0 = (rng.random(card_of(3, K, 0)) < 0.6).astype(np.uint8)
    m2 = (rng.random(CARD[2]) < 0.6).astype(np.uint8)
    want = reference(d, [(0, m0), (2, m2)])
    assert 0 < want.sum() < K
    # one device block: [shift bytes | m0 | m2 | pad], another for the output: [shift bytes | K bytes | guard]
    blob = np.zeros(64, np.uint8)
    blob[shift:shift + m0.size] = m0
    blob[shift + m0.size:shift + m0.size + m2.size] = m2
    dm = DeviceArray.from_host(engine, blob.view(np.uint64))
    out = DeviceArray.from_host(engine, np.full((K + 16 + 7) // 8, 0x7777777777777777, np.uint64))
    n_sel = raw_select(engine, d, [(0, m0), (2, m2)], out.ptr + shift, memory=capi.TAD_MEM_DEVICE, keep_len=K,
                       mask_ptrs=[dm.ptr + shift, dm.ptr + shift + m0.size], mask_lens=[m0.size, m2.size])
    got = out.to_host().view(np.uint8)
    assert np.array_equal(got[shift:shift + K], want) and n_sel == int(want.sum())
    assert (got[:shift] == 0x77).all() and (got[shift + K:] == 0x77).all()       # nothing written outside key_keep
    # the wrapper's device form: DeviceArray masks in, a DeviceArray of bytes out
    keep, n2 = d.select([(0, dm.view(shift, m0.size, np.uint8)), (2, dm.view(shift + m0.size, m2.size, np.uint8))], out="device")
    assert isinstance(keep, DeviceArray) and keep.n == K and np.array_equal(keep.to_host(), want) and n2 == n_sel
    d.close()


# ---- 5. refusals: the dictionary exports the same bytes afterwards ----
def test_refusals_leave_the_dictionary_unchanged(engine):
    K = 300
    d = filled(engine, 3, K)
    snap = keydict_snapshot(d)
    m = np.ones(card_of(3, K, 0), np.uint8)
    good = np.zeros(K, np.uint8)
    assert raw_select(engine, d, [(0, m)], good) == K
    cases = {"key_keep_len too short": dict(keep=np.zeros(K - 1, np.uint8)), "key_keep_len too long": dict(keep=np.zeros(K + 1, np.uint8)),
             "term_col == n_cols": dict(cols=[3]), "term_col negative": dict(cols=[-1]), "side 2": dict(side=2), "side -2": dict(side=-2),
             "n_terms 9": dict(n_terms=9, terms=[(0, m)] * 9), "n_terms negative": dict(n_terms=-1),
             "key_keep NULL": dict(keep=0, keep_len=K), "memory 7": dict(memory=7)}
    for name, kw in cases.items():
        terms = kw.pop("terms", [(0, m)])
        keep = kw.pop("keep", good)
        with pytest.raises(TadError) as ei:
            raw_select(engine, d, terms, keep, **kw)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT, name
        assert "tad_keydict_select" in ei.value.message, (name, ei.value.message)
        assert_keydict_unchanged(d, snap, name)
    # a tuple value equal to mask_len: the mask of column 0 one byte short of the largest code the dictionary holds
    cols, _ = d.export()
    top = int(cols[0].max())
    assert top > 0 and (cols[0] == top).any()
    for out in ("host", "device"):
        with pytest.raises(TadError) as ei:
            d.select([(0, np.ones(top, np.uint8))], out=out)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "outside the mask" in ei.value.message
        assert_keydict_unchanged(d, snap, "value == mask_len")
    assert raw_select(engine, d, [(0, m)], good) == K and good.all()          # the next call is served
    d.close()
    # a negative tuple value
    d = engine.key_dict(2, expected_keys=1)
    d.encode([np.array([0, 1, -1, 2], np.int64), np.array([0, 0, 0, 0], np.int64)])
    snap = keydict_snapshot(d)
    with pytest.raises(TadError) as ei:
        d.select([(0, np.ones(8, np.uint8))], out="host")
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "outside the mask" in ei.value.message
    assert_keydict_unchanged(d, snap, "negative value")
    keep, n_sel = d.select([(1, np.ones(1, np.uint8))], out="host")           # the other column is in range
    assert n_sel == 4 and keep.all()
    d.close()


def test_empty_dictionary(engine):
    d = engine.key_dict(2, expected_keys=1)
    for out in ("host", "device"):
        keep, n_sel = d.select([(0, np.ones(4, np.uint8))], out=out)
        assert n_sel == 0 and host_of(keep).size == 0
    assert raw_select(engine, d, [], np.zeros(0, np.uint8)) == 0
    with pytest.raises(TadError):
        raw_select(engine, d, [], np.zeros(1, np.uint8))
    d.close()
