"""GPU: the four ingest encoders — tad_factorize and tad_encode_strings (the keys of one call), tad_keydict and tad_strdict (ids that outlive
the call) — share their slot table (tad_slots.h) and their host plumbing (tad_capi_dict.h).  What must not move when that plumbing does:
the texts of their refusals, byte for byte (the workspace-limit ones carry the scratch byte count, so they pin the staging layout), a
dictionary that a refused call leaves as it was, and the numbering: a dictionary that starts empty numbers a batch exactly as the one-call
encoder does, bit for bit, through a table that grows inside the call.  The expected texts were recorded from the library of before the
encoders shared these pieces."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadEngine, TadError
from theia_amd import _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import column, host

pytestmark = pytest.mark.gpu

U64 = np.uint64
N_BIG = 100_000

WORKSPACE_REFUSALS = {
    "tad_factorize, device": b"tad_factorize needs 2547968 bytes of scratch > workspace limit 1048576",
    "tad_encode_strings, device": b"tad_encode_strings needs 2547968 bytes of scratch > workspace limit 1048576",
    "tad_keydict_encode, device": b"tad_keydict_encode needs 4248320 bytes of scratch > workspace limit 1048576",
    "tad_keydict_encode, host": b"tad_keydict_encode needs 2700544 bytes of scratch > workspace limit 1048576",
    "tad_strdict_encode, device": b"tad_strdict_encode needs 4649104 bytes of scratch > workspace limit 1048576 (dictionary unchanged)",
    "tad_strdict_encode, host": b"tad_strdict_encode needs 2100736 bytes of scratch > workspace limit 1048576",
}

ARGUMENT_REFUSALS = {
    "n_cols": b"tad_keydict_encode: 2 key columns, the dictionary holds tuples of 3",
    "null column": b"tad_keydict_encode: key column 1 is NULL",
    "offsets decrease": b"tad_strdict_encode: offsets decrease or point beyond data_bytes (dictionary unchanged)",
    "offset beyond data": b"tad_strdict_encode: offsets decrease or point beyond data_bytes (dictionary unchanged)",
    "keydict import, duplicate": b"tad_keydict_import: two keys hold the same tuple (dictionary unchanged)",
    "strdict import, duplicate": b"tad_strdict_import: two strings are equal (3 distinct of 4; dictionary unchanged)",
    "keydict import, not empty": b"tad_keydict_import: the dictionary holds 100 keys (import fills an empty one)",
    "strdict import, not empty": b"tad_strdict_import: the dictionary holds 50 values (import fills an empty one)",
    "compact, wrong length": b"tad_keydict_compact: remap has 99 entries, the dictionary holds 100 keys (dictionary unchanged)",
    "compact, out of order": b"tad_keydict_compact: the entries of remap that are not TAD_KEY_SKIP must be 0, 1, ..., m - 1 in order (what tad_state_compact writes); dictionary unchanged",
    "select, stale length": b"tad_keydict_select: key_keep has 99 entries, the dictionary holds 100 keys",
    "match, long pattern": b"tad_strdict_match: bad arguments (dictionary, op TAD_STR_EQUAL / TAD_STR_CONTAINS_NOCASE, a pattern of at most 1024 bytes, mask in host or device memory)",
}


def last_error(engine):
    return bytes(engine._lib.tad_last_error(engine._h))


def refused(engine, code, call, *args, **kw):
    """-> tad_last_error after `call` was refused with `code`"""
    with pytest.raises(TadError) as ei:
        call(*args, **kw)
    assert ei.value.code == code, ei.value
    return last_error(engine)


def device_column(engine, col):
    off, data = col
    room = DeviceArray.from_host(engine, np.concatenate([data, np.zeros(16, np.uint8)]))      # (the last aligned word a kernel loads)
    return DeviceArray.from_host(engine, off), room.view(0, data.size, np.uint8)


def dev(engine, cols):
    return [DeviceArray.from_host(engine, np.ascontiguousarray(c)) for c in cols]


# ---- 1. the workspace-limit refusals: the text carries the scratch bytes of the staging layout ----
def workspace_refusals(small):
    big = [np.arange(N_BIG, dtype=np.int64) + 5000, np.arange(N_BIG, dtype=np.int64)]
    strings = column([b"%08d" % i for i in range(N_BIG)])
    grid = capi.TAD_ERR_GRID_TOO_LARGE
    seen = {}
    seen["tad_factorize, device"] = refused(small, grid, small.factorize, dev(small, big))
    seen["tad_encode_strings, device"] = refused(small, grid, small.encode_strings, device_column(small, strings))
    kd, sd = small.key_dict(2, 1), small.string_dict(1, 1)
    seen["tad_keydict_encode, device"] = refused(small, grid, kd.encode, dev(small, big))
    seen["tad_keydict_encode, host"] = refused(small, grid, kd.encode, big)
    seen["tad_strdict_encode, device"] = refused(small, grid, sd.encode, device_column(small, strings), out="device")
    seen["tad_strdict_encode, host"] = refused(small, grid, sd.encode, strings)
    assert kd.num_keys() == 0 and sd.num_values() == 0
    kd.close()
    sd.close()
    return seen


def test_the_workspace_limit_refusals_keep_their_text_and_their_byte_counts(engine):
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    try:
        seen = workspace_refusals(small)
    finally:
        small.close()
    assert sorted(seen) == sorted(WORKSPACE_REFUSALS)
    for case in sorted(seen):
        print(case, seen[case])
    for case in sorted(WORKSPACE_REFUSALS):
        assert seen[case] == WORKSPACE_REFUSALS[case], (case, seen[case])


# ---- 2. the argument refusals: their text, and the dictionary as it was ----
def kd_snapshot(d):
    cols, side = d.export()
    return d.num_keys(), [c.tobytes() for c in cols], side.tobytes()


def sd_snapshot(d):
    off, data = d.export()
    return d.num_values(), off.tobytes(), data.tobytes()


def kd_encode_raw(engine, d, n_cols, cols, n):
    arr = (C.c_void_p * len(cols))(*[None if c is None else c.ctypes.data for c in cols])
    kc = capi.KeyColumns(n_rows=n, n_cols=n_cols, cols_a=arr, keep_a=None, cols_b=None, keep_b=None, memory=capi.TAD_MEM_HOST)
    k1, fr = np.zeros(n, U64), np.zeros(n, U64)
    before, after = capi.u64(), capi.u64()
    return engine._lib.tad_keydict_encode(engine._h, d._h, C.byref(kc), k1.ctypes.data, None, fr.ctypes.data, n, C.byref(before), C.byref(after))


def sd_encode_raw(engine, d, off, data):
    n = off.size - 1
    codes, first = np.zeros(n, np.int64), np.zeros(n, U64)
    sc = capi.StringColumn(n_rows=n, offsets=off.ctypes.data, offset_bits=32, data=data.ctypes.data, data_bytes=data.size, validity=None, validity_offset=0,
                           memory=capi.TAD_MEM_HOST)
    before, after = capi.u64(), capi.u64()
    return engine._lib.tad_strdict_encode(engine._h, d._h, C.byref(sc), codes.ctypes.data, first.ctypes.data, n, C.byref(before), C.byref(after))


def argument_refusals(engine):
    """-> ({case: tad_last_error}, {case: the dictionary is as it was})"""
    inv = capi.TAD_ERR_INVALID_ARGUMENT
    lib = engine._lib
    seen, same = {}, {}
    cols = [np.arange(100, dtype=np.int64) + 1000 * i for i in range(3)]
    kd = engine.key_dict(3, 1)
    kd.encode(cols)
    sd = engine.string_dict(1, 1)
    sd.encode(column([b"held-%d" % i for i in range(50)]))
    kd_snap, sd_snap = kd_snapshot(kd), sd_snapshot(sd)

    def note(case, d=None):
        seen[case] = last_error(engine)
        same[case] = kd_snapshot(kd) == kd_snap and sd_snapshot(sd) == sd_snap if d is None else d

    new = [c + 500 for c in cols]
    assert kd_encode_raw(engine, kd, 2, new[:2], 100) == inv
    note("n_cols")
    assert kd_encode_raw(engine, kd, 3, [new[0], None, new[2]], 100) == inv
    note("null column")
    # 300 rows of new strings; the bad offset lies at row 257, in the probe's second workgroup
    off, data = column([b"new-%d" % i for i in range(300)])
    bad = off.copy()
    bad[257] = bad[256] - 2
    assert sd_encode_raw(engine, sd, bad, data) == inv
    note("offsets decrease")
    bad = off.copy()
    bad[-1] += 40
    assert sd_encode_raw(engine, sd, bad, data) == inv
    note("offset beyond data")
    # imports: into an empty dictionary with a duplicate, and into one that holds something
    kd2, sd2 = engine.key_dict(3, 1), engine.string_dict(1, 1)
    dup = [np.array([1, 2, 3, 2], dtype=np.int64)] * 3
    seen["keydict import, duplicate"] = refused(engine, inv, kd2.load, dup)
    same["keydict import, duplicate"] = kd2.num_keys() == 0
    seen["strdict import, duplicate"] = refused(engine, inv, sd2.load, [b"a", b"b", b"c", b"b"])
    same["strdict import, duplicate"] = sd2.num_values() == 0
    kd2.close()
    sd2.close()
    seen["keydict import, not empty"] = refused(engine, inv, kd.load, cols)
    note("keydict import, not empty")
    seen["strdict import, not empty"] = refused(engine, inv, sd.load, [b"x"])
    note("strdict import, not empty")
    remap = np.arange(100, dtype=U64)
    seen["compact, wrong length"] = refused(engine, inv, kd.compact, remap[:99])
    note("compact, wrong length")
    swapped = remap.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    seen["compact, out of order"] = refused(engine, inv, kd.compact, swapped)
    note("compact, out of order")
    keep = np.zeros(100, np.uint8)
    n_sel = capi.u64()
    assert lib.tad_keydict_select(engine._h, kd._h, 0, None, None, None, -1, keep.ctypes.data, 99, capi.TAD_MEM_HOST, C.byref(n_sel)) == inv
    note("select, stale length")
    seen["match, long pattern"] = refused(engine, inv, sd.match, capi.TAD_STR_EQUAL, b"p" * 1025)
    note("match, long pattern")
    kd.close()
    sd.close()
    return seen, same


def test_the_argument_refusals_keep_their_text_and_leave_the_dictionary_unchanged(engine):
    seen, same = argument_refusals(engine)
    assert sorted(seen) == sorted(ARGUMENT_REFUSALS)
    for case in sorted(seen):
        print(case, seen[case])
    for case in sorted(ARGUMENT_REFUSALS):
        assert seen[case] == ARGUMENT_REFUSALS[case], (case, seen[case])
        assert same[case], case


# ---- 3. two spellings of one numbering ----
@pytest.mark.parametrize("memory", ["host", "device"])
def test_an_empty_key_dictionary_numbers_a_batch_as_factorize_does(engine, memory):
    """3 columns, two sides, 700 rows over 90 distinct tuples.  The dictionary's first table has 64 slots: 90 new keys grow it inside the
    call, so both the append and the rehash claim slots."""
    rng = np.random.default_rng(44)
    tuples = np.stack([rng.integers(-5, 6, size=90) * 977, np.arange(90) + (1 << 40), rng.integers(0, 3, size=90)]).astype(np.int64)
    pick_a, pick_b = rng.integers(0, 90, size=700), rng.integers(0, 90, size=700)
    a, b = [np.ascontiguousarray(tuples[c][pick_a]) for c in range(3)], [np.ascontiguousarray(tuples[c][pick_b]) for c in range(3)]
    assert len({(int(s),) + tuple(int(x[i]) for x in cols) for s, cols in ((0, a), (1, b)) for i in range(700)}) > 64
    ca, cb = (dev(engine, a), dev(engine, b)) if memory == "device" else (a, b)
    want1, want2, want_first = engine.factorize(ca, None, cb, None)
    d = engine.key_dict(3, 1)
    k1, k2, first, before = d.encode(ca, None, cb, None)
    assert before == 0 and d.num_keys() == host(want_first).size > 64
    assert isinstance(k1, DeviceArray) == (memory == "device")
    assert host(k1).tobytes() == host(want1).tobytes() and host(k2).tobytes() == host(want2).tobytes()
    assert host(first).tobytes() == host(want_first).tobytes()
    d.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_an_empty_string_dictionary_numbers_a_batch_as_encode_strings_does(engine, memory):
    """700 rows over 90 distinct strings of 0 .. 40 bytes, into a dictionary of the smallest table and arena: all three grow inside the call"""
    rng = np.random.default_rng(45)
    vocab = [bytes(rng.integers(97, 123, size=i % 41, dtype=np.uint8)) + b"%d" % i if i else b"" for i in range(90)]
    vocab = [v[:40] for v in vocab]
    assert len(set(vocab)) == 90 and {len(v) for v in vocab} >= {0, 40}
    col = column([vocab[i] for i in rng.integers(0, 90, size=700)])
    arg = device_column(engine, col) if memory == "device" else col
    want_codes, want_first = engine.encode_strings(arg)
    d = engine.string_dict(1, 1)
    codes, first, before = d.encode(arg, out=memory)
    assert before == 0 and d.num_values() == host(want_first).size
    assert isinstance(codes, DeviceArray) == (memory == "device")
    assert host(codes).tobytes() == host(want_codes).tobytes()
    assert host(first).tobytes() == host(want_first).tobytes()
    d.close()
