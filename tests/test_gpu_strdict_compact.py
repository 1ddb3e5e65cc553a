"""GPU: tad_strdict_compact (include/tad.h, TAD_FEATURE_STRING_RETIRE) — values leave a string dictionary, the survivors are renumbered
densely and the arena is packed.  The model is a Python list: survivors = [v for c, v in enumerate(values) if keep[c]].  After every
compaction the dictionary is compared, call by call, with a FRESH StringDict loaded with the survivors and with the list itself: remap, the
export, num_values, the lookup of every old value, a decode of shuffled codes, both match operations, an encode that mixes retired, surviving
and new strings, and every field of the stats.  Every comparison is exact.  The shapes sit on the edges the kernels have: the workgroup of
256 values (kSdBlock) for the flag, record and copy kernels, the scan's tile, survivor counts on the copy's own workgroup edge, string
lengths around the 16-byte word, and a survivor longer than one workgroup pass of the copy (kSdCopyLaneMax words)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import ROOT, column, exported, hash8, host

pytestmark = pytest.mark.gpu

LENGTHS = (15, 16, 17, 31, 32, 33, 127, 128, 129)      # (0 and 1 are placed by hand: few strings are that short)


def _source_constants():
    sd = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_strdict.hip")).read()
    kern = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_kernels.hip")).read()
    block = int(re.search(r"static constexpr int kSdBlock = (\d+);", sd).group(1))
    assert re.search(r"static constexpr uint32_t kSdCopyLaneMax = kSdBlock;", sd)
    kblock = int(re.search(r"static constexpr int kBlock = (\d+);", kern).group(1))
    items = int(re.search(r"static constexpr int kScanItems = (\d+);", kern).group(1))
    assert re.search(r"kScanTile = kBlock \* kScanItems;", kern)
    return block, kblock * items


BLOCK, SCAN_TILE = _source_constants()
COUNTS = [1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1]


def test_the_shapes_sit_on_the_kernels_edges():
    assert BLOCK == 256 and SCAN_TILE == 2048
    assert COUNTS == [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]


def up16(n):
    return (n + 15) & ~15


def make_values(n, seed):
    """n distinct strings of mixed lengths; the empty string, a few one-byte strings and every length of LENGTHS are among them when n allows"""
    rng = np.random.default_rng(seed)
    vals = []
    for i in range(n):
        L = LENGTHS[i % len(LENGTHS)] if i < 2 * len(LENGTHS) else LENGTHS[int(rng.integers(len(LENGTHS)))]
        vals.append(i.to_bytes(4, "little") + rng.integers(0, 256, L - 4, dtype=np.uint8).tobytes())
    for k, pos in enumerate((n // 3, n // 2 + 1, n - 2)):
        if 0 < pos < n and n > 8:
            vals[pos] = bytes([65 + k])                  # one byte
    if n > 4:
        vals[n // 4] = b""
    assert len(set(vals)) == n
    return vals


def keep_pattern(name, n, seed=0):
    k = np.zeros(n, dtype=np.uint8)
    if name == "all":
        k[:] = 1
    elif name == "first":
        k[0] = 1
    elif name == "last":
        k[-1] = 1
    elif name == "alternating":
        k[::2] = 1
    elif name == "run":                                   # one dropped run of two workgroups' worth and a bit, not on a workgroup's edge
        k[:] = 1
        lo = min(BLOCK // 2 + 3, n // 4)
        k[lo:min(lo + 2 * BLOCK + 5, n - 1)] = 0
    elif name == "half":
        k[:] = np.random.default_rng(1000 + seed).integers(0, 2, n)
    elif name == "one64th":
        k[:] = np.random.default_rng(2000 + seed).integers(0, 64, n) == 0
    else:
        assert name == "none"
    return k


def filled(engine, values, batch=None):
    d = engine.string_dict(1, 1)
    step = batch or max(len(values), 1)
    for i in range(0, len(values), step):
        codes = d.encode(column(values[i:i + step], 64))[0]
        assert np.array_equal(codes, np.arange(i, min(i + step, len(values))))
    return d


def check_compact(engine, d, values, keep, keep_arg=None, out="host", extra=None):
    """compact d (which holds `values`) with keep and compare it with the model and with a fresh dictionary of the survivors; returns the
    survivors (d then holds them, and the strings of the mixed encode behind them)"""
    keep = np.asarray(keep, dtype=np.uint8)
    survivors = [v for c, v in enumerate(values) if keep[c]]
    m = len(survivors)
    want_remap = np.where(keep != 0, np.cumsum(keep != 0) - 1, -1).astype(np.int64)
    nbytes_before = d.nbytes()
    remap, st = d.compact(keep if keep_arg is None else keep_arg, out=out)
    assert isinstance(remap, DeviceArray) == (out == "device")
    assert np.array_equal(host(remap), want_remap)
    fresh = engine.string_dict(1, 1)
    fresh.load(survivors)
    # the values held
    assert d.num_values() == m == fresh.num_values()
    assert exported(d) == survivors == exported(fresh)
    # every stats field
    assert (st["values_before"], st["values_after"]) == (len(values), m)
    assert (st["bytes_before"], st["bytes_after"]) == (nbytes_before, d.nbytes()) and d.nbytes() <= nbytes_before
    assert st["arena_used_before"] == sum(up16(len(v)) for v in values) and st["arena_used_after"] == sum(up16(len(v)) for v in survivors)
    assert st["job_context"] >= 0 and st["ms_total"] >= 0.0
    if m == len(values):
        assert st["bytes_after"] == st["bytes_before"]                       # nothing retired: nothing reallocated
    # lookup of every old value: the new code, or TAD_CODE_NONE
    if values:
        assert np.array_equal(d.lookup(column(values, 64)), want_remap)
        assert np.array_equal(fresh.lookup(column(values, 64)), want_remap)
    # decode of a shuffled code list
    if m:
        codes = np.random.default_rng(m).integers(0, m, min(3 * m + 1, 3000)).astype(np.int64)
        got, ref = d.decode(codes), fresh.decode(codes)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(got[0], np.concatenate([[0], np.cumsum([len(survivors[c]) for c in codes])]))
    # both match operations
    pat = next((v for v in survivors[m // 2:] + survivors if len(v) <= 1024), b"x")      # (a pattern has at most 1024 bytes)
    for op, p, rule in ((capi.TAD_STR_EQUAL, pat, lambda v: v == pat), (capi.TAD_STR_CONTAINS_NOCASE, b"a", lambda v: b"a" in v.lower())):
        mask, hit = d.match(op, p)
        fmask, fhit = fresh.match(op, p)
        want = np.array([1 if rule(v) else 0 for v in survivors], dtype=np.uint8)
        assert np.array_equal(mask, want) and np.array_equal(fmask, want) and hit == fhit == int(want.sum())
    # an encode that mixes retired, surviving and new strings: new codes m, m + 1, ... in order of first appearance
    retired = [v for c, v in enumerate(values) if not keep[c]]
    new = extra if extra is not None else [b"new-%d" % i for i in range(5)]
    batch = retired[:7] + survivors[:9] + new + retired[:3] + survivors[-2:] + new[:2]
    seen, want_codes = {v: i for i, v in enumerate(survivors)}, []
    for v in batch:
        want_codes.append(seen.setdefault(v, len(seen)))
    if batch:
        got, ref = d.encode(column(batch, 64)), fresh.encode(column(batch, 64))
        assert np.array_equal(got[0], want_codes) and np.array_equal(ref[0], want_codes)
        assert np.array_equal(got[1], ref[1]) and got[2] == ref[2] == m
        assert exported(d) == sorted(seen, key=seen.get) == exported(fresh)
    fresh.close()
    return sorted(seen, key=seen.get)


PATTERNS = ["all", "none", "first", "last", "alternating", "run", "half", "one64th"]


@pytest.mark.parametrize("n,pattern", [(n, p) for n in COUNTS for p in PATTERNS if p != "run" or n >= 3 * BLOCK])      # (the run spans two workgroups' worth)
def test_every_value_count_and_keep_pattern(engine, n, pattern):
    values = make_values(n, n)
    d = filled(engine, values)
    check_compact(engine, d, values, keep_pattern(pattern, n, n))
    d.close()


@pytest.mark.parametrize("m", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1])
def test_survivor_counts_on_the_copy_workgroup_edge(engine, m):
    """the copy takes 256 consecutive SURVIVORS per workgroup, whatever the old count: 2049 values, every 7th or so kept"""
    n = SCAN_TILE + 1
    values = make_values(n, 7 * m)
    keep = np.zeros(n, dtype=np.uint8)
    keep[np.sort(np.random.default_rng(m).choice(n, m, replace=False))] = 1
    d = filled(engine, values)
    check_compact(engine, d, values, keep)
    d.close()


@pytest.mark.parametrize("where", ["first", "middle", "last", "only", "dropped"])
def test_the_empty_string_as_a_survivor(engine, where):
    """a row of no bytes shares its destination offset with its successor: the copy's search passes over it, the table still holds it"""
    body = [b"k%03d" % i + b"x" * (i % 40) for i in range(300)]
    values = {"first": [b""] + body, "middle": body[:150] + [b""] + body[150:], "last": body + [b""], "only": body[:5] + [b""] + body[5:],
              "dropped": body[:150] + [b""] + body[150:]}[where]
    keep = np.ones(len(values), dtype=np.uint8)
    keep[1::3] = 0
    e = values.index(b"")
    keep[e] = 0 if where == "dropped" else 1
    if where == "only":
        keep[:] = 0
        keep[e] = 1
    d = filled(engine, values)
    check_compact(engine, d, values, keep)
    d.close()


@pytest.mark.parametrize("lengths", [(0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129)])
def test_every_string_length_around_the_word(engine, lengths):
    values = [b""] + [bytes([1 + i]) * L for i, L in enumerate(lengths) if L]
    for pattern in ("all", "alternating", "none"):
        d = filled(engine, values)
        check_compact(engine, d, values, keep_pattern(pattern, len(values)))
        d.close()
    keep = np.ones(len(values), dtype=np.uint8)
    keep[0] = 0                                            # odd survivors this time
    keep[2::2] = 0
    d = filled(engine, values)
    check_compact(engine, d, values, keep)
    d.close()


@pytest.mark.parametrize("big_kept", [True, False])
def test_one_string_of_70000_bytes_among_short_ones(engine, big_kept):
    """4375 words: far over one workgroup pass (kSdCopyLaneMax = 256 words), so the wavefronts copy it while the lanes walk the short rows"""
    big = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    values = [b"short-%d" % i for i in range(40)] + [big] + [b"after-%d" % i for i in range(40)]
    keep = np.ones(len(values), dtype=np.uint8)
    keep[3::4] = 0
    keep[40] = 1 if big_kept else 0
    d = filled(engine, values)
    check_compact(engine, d, values, keep)
    d.close()


def test_survivors_around_one_workgroup_pass_of_the_copy(engine):
    """4096 bytes are 256 words, the most a lane-walked row has; 4097 bytes are 257 words and go to the wavefronts.  Several long rows in one
    tile (more than the four wavefronts), long rows first and last in the tile, and short rows between them"""
    rng = np.random.default_rng(9)
    lens = [4097, 20, 4080, 4096, 0, 4097, 4112, 33, 8192, 5000, 16, 4100, 9000, 4096, 4097]
    values = [i.to_bytes(2, "little") + rng.integers(0, 256, max(L - 2, 0), dtype=np.uint8).tobytes() if L else b"" for i, L in enumerate(lens)]
    for keep in (np.ones(len(values), np.uint8), keep_pattern("alternating", len(values)), 1 - keep_pattern("alternating", len(values))):
        d = filled(engine, values)
        check_compact(engine, d, values, keep)
        d.close()


def test_a_tile_of_256_survivors_far_larger_than_any_stage(engine):
    """600 values of 129 .. 328 bytes: a workgroup's 256 survivors move about 58 KiB, several passes of the walk over the LDS offsets"""
    values = [b"%04d" % i + bytes([32 + i % 90]) * (125 + i % 200) for i in range(600)]
    keep = np.ones(600, dtype=np.uint8)
    keep[5::11] = 0
    d = filled(engine, values)
    check_compact(engine, d, values, keep)
    d.close()


@pytest.fixture(scope="module")
def fingerprint_pair():
    """two 8-byte strings whose hashes share the high 32 bits, the slot's fingerprint (among 4e5 strings 18.6 such pairs are expected)"""
    words = np.arange(400000, dtype=np.uint64) * np.uint64(0x0101010101010101) + np.uint64(0x2020202020202020)
    fp = hash8(words) >> np.uint64(32)
    order = np.argsort(fp, kind="stable")
    same = np.flatnonzero(fp[order][1:] == fp[order][:-1])
    assert same.size > 0
    a, b = words[order[same[0]]].tobytes(), words[order[same[0] + 1]].tobytes()
    assert a != b
    return a, b


@pytest.mark.parametrize("kept", ["both", "first", "second"])
def test_two_strings_with_one_fingerprint(engine, fingerprint_pair, kept):
    """the fresh table is filled from the old slots' fingerprints and the records' low halves: the pair must stay two values, and the one
    that stays must not answer for the one that left"""
    a, b = fingerprint_pair
    values = [b"before", a, b"between", b, b"after"]
    keep = np.array([1, kept != "second", 0, kept != "first", 1], dtype=np.uint8)
    d = filled(engine, values)
    check_compact(engine, d, values, keep, extra=[b"n1", a, b, b"n2"])
    d.close()


def test_a_dictionary_that_grew_shrinks_and_grows_again(engine):
    n = 70_000
    values = [b"pod-%08d-%s" % (i, b"abcdefghij"[:i % 11]) for i in range(n)]
    d = filled(engine, values)
    before = d.nbytes()
    keep = np.zeros(n, dtype=np.uint8)
    keep[np.sort(np.random.default_rng(3).choice(n, 100, replace=False))] = 1
    survivors = [v for c, v in enumerate(values) if keep[c]]
    held = check_compact(engine, d, values, keep)
    # the sizes tad_strdict_create(200, 2 x the survivors' padded bytes) picks
    held_bytes = sum(up16(len(v)) for v in survivors)
    assert d.nbytes() < before
    # (check_compact's encode has appended to it since; it took the stats' bytes_after before that)
    d2 = filled(engine, values)
    _, st = d2.compact(keep)
    assert st["bytes_after"] == 512 * 8 + 200 * 16 + 2 * held_bytes < st["bytes_before"] == before
    d2.close()
    # later growth works again: records, arena and table all pass their new capacity
    more = [b"later-%d" % i for i in range(5000)]
    codes, first, nb = d.encode(column(more + held[:50], 64))
    assert nb == len(held) and np.array_equal(codes, np.concatenate([len(held) + np.arange(5000), np.arange(50)]))
    assert exported(d) == held + more
    d.close()


def test_refusals_leave_the_dictionary_unchanged(engine):
    values = make_values(300, 42)
    d = filled(engine, values)
    snap = (exported(d), d.nbytes())
    for bad in (299, 301, 0):
        with pytest.raises(TadError) as ei:
            d.compact(np.ones(bad, np.uint8))
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "300" in ei.value.message
        assert (exported(d), d.nbytes()) == snap
    lib, keep = engine._lib, np.zeros(300, np.uint8)
    remap = np.full(300, 77, dtype=np.int64)
    rc = lib.tad_strdict_compact(engine._h, d._h, keep.ctypes.data, 300, capi.TAD_MEM_HOST, None, capi.TAD_MEM_HOST, None)      # NULL remap
    assert rc == capi.TAD_ERR_INVALID_ARGUMENT and (exported(d), d.nbytes()) == snap
    assert lib.tad_strdict_compact(engine._h, d._h, None, 300, capi.TAD_MEM_HOST, remap.ctypes.data, capi.TAD_MEM_HOST, None) == capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_strdict_compact(engine._h, d._h, keep.ctypes.data, 300, 7, remap.ctypes.data, capi.TAD_MEM_HOST, None) == capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_strdict_compact(engine._h, None, keep.ctypes.data, 300, capi.TAD_MEM_HOST, remap.ctypes.data, capi.TAD_MEM_HOST, None) == capi.TAD_ERR_INVALID_ARGUMENT
    assert (remap == 77).all() and (exported(d), d.nbytes()) == snap
    check_compact(engine, d, values, keep_pattern("half", 300))             # and it still compacts
    d.close()


def test_workspace_limit_refuses_the_scans_and_leaves_the_dictionary_unchanged():
    """32 B a value of scratch (flags, units, two scans, the old offsets): 40 000 values need 1.28 MB and are refused under a limit of
    1 MiB — before anything is allocated or moved; 20 000 values pass"""
    small = TadEngine(device=0, workspace_limit=1 << 20)
    try:
        values = [b"value-%06d" % i for i in range(40_000)]
        d = filled(small, values, batch=1000)
        snap = (exported(d), d.nbytes())
        keep = DeviceArray.from_host(small, np.frombuffer(keep_pattern("half", 40_000).tobytes(), dtype=np.uint64)).view(0, 40_000, np.uint8)
        with pytest.raises(TadError) as ei:
            d.compact(keep, out="device")
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE and "unchanged" in ei.value.message
        assert (exported(d), d.nbytes()) == snap
        d.close()
        d = filled(small, values[:20_000], batch=1000)
        keep = keep_pattern("half", 20_000)
        remap, st = d.compact(DeviceArray.from_host(small, np.frombuffer(keep.tobytes(), dtype=np.uint64)).view(0, 20_000, np.uint8), out="device")
        assert exported(d) == [v for c, v in enumerate(values[:20_000]) if keep[c]] and st["values_after"] == int(keep.sum())
        d.close()
    finally:
        small.close()


@pytest.mark.parametrize("keep_mem,out", [("host", "host"), ("host", "device"), ("device", "host"), ("device", "device"), ("misaligned", "device")])
def test_host_and_device_keep_and_remap(engine, keep_mem, out):
    n = SCAN_TILE + 77
    values = make_values(n, 11)
    keep = keep_pattern("half", n, 5)
    arg, base = keep, None
    if keep_mem != "host":
        shift = 3 if keep_mem == "misaligned" else 0
        padded = np.concatenate([np.full(shift, 0xEE, np.uint8), keep, np.full(-(shift + n) % 8, 0xEE, np.uint8)])
        base = DeviceArray.from_host(engine, np.frombuffer(padded.tobytes(), dtype=np.uint64))
        arg = base.view(shift, n, np.uint8)
        assert (arg.ptr % 8 == 3) == (keep_mem == "misaligned")
    d = filled(engine, values)
    check_compact(engine, d, values, keep, keep_arg=arg, out=out)
    d.close()


@pytest.mark.parametrize("dtype,lo", [(np.int64, 256), (np.int32, 65536), (np.float64, 0.5), (np.int16, -256), (bool, True)])
def test_a_host_keep_of_any_type_keeps_what_is_not_zero(engine, dtype, lo):
    """survives iff keep[c] != 0: a value whose low byte is 0, or a fraction, is not 0"""
    values = [b"v%d" % i for i in range(20)]
    keep = np.zeros(20, dtype=dtype)
    keep[[1, 5, 19]] = lo
    d = filled(engine, values)
    remap, st = d.compact(keep)
    assert exported(d) == [values[1], values[5], values[19]] and st["values_after"] == 3
    d.close()


def test_twice_in_a_row_then_an_import_into_the_emptied_dictionary(engine):
    values = make_values(1000, 77)
    d = filled(engine, values)
    held = check_compact(engine, d, values, keep_pattern("half", 1000))
    held = check_compact(engine, d, held, keep_pattern("alternating", len(held)), extra=[b"again-%d" % i for i in range(4)])
    before = d.nbytes()
    remap, st = d.compact(np.zeros(len(held), np.uint8))
    assert (remap == -1).all() and d.num_values() == 0 and exported(d) == []
    # the minimum sizes of tad_strdict_create: 64 slots, 32 records, 16 bytes of arena
    assert st["bytes_after"] == d.nbytes() == 64 * 8 + 32 * 16 + 16 <= before and st["arena_used_after"] == 0
    remap, st = d.compact(np.zeros(0, np.uint8))                             # an empty dictionary: nothing to do
    assert remap.size == 0 and st["values_before"] == 0 and d.nbytes() == 64 * 8 + 32 * 16 + 16
    again = [b"imported-%d" % i for i in range(500)]
    d.load(again)
    assert exported(d) == again and np.array_equal(d.lookup(column(again[::-1], 64)), np.arange(500)[::-1])
    check_compact(engine, d, again, keep_pattern("one64th", 500))
    d.close()
