"""GPU: LIKE patterns with % and _ on the persistent string dictionary (tad_strdict_like, include/tad.h; kernel k_sd_like).  Every mask is
compared bit for bit with the plain-Python matcher of tests/like_ref.py, with and without TAD_LIKE_NOCASE, through the host mask and the
device mask, and n_matched with the mask's sum.  The dictionaries start at the smallest table and arena (expected_values=1,
expected_bytes=1).  Shapes: value lengths around every 8- and 16-byte word of the arena with the matching text at every word edge, _ over
2-, 3- and 4-byte characters across an edge, malformed UTF-8, the pattern table of the host test, the longest pattern, value counts around
the wavefront and the workgroup, and one dictionary of one value more than the kernel's grid holds lanes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import like_ref
from theia_amd import TadError, _capi as capi
from job_helpers import ROOT, column

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257)
COUNTS = (1, 63, 64, 65, 255, 256, 257)


def held(engine, values):
    """a dictionary whose value c is values[c] (distinct byte strings)"""
    assert len(set(values)) == len(values)
    d = engine.string_dict(1, 1)
    codes = d.encode(column(values, 64))[0]
    assert np.array_equal(codes, np.arange(len(values)))
    return d


def check(d, values, pattern, flags=(False, True)):
    """both flags, both memories, the count; returns the matches of the last flag (without case)"""
    pattern = pattern.encode() if isinstance(pattern, str) else pattern
    hits = None
    for nocase in flags:
        want = np.array(like_ref.like_mask(pattern, values, nocase), dtype=np.uint8)
        mask, n = d.like(pattern, nocase=nocase)
        assert mask.dtype == np.uint8 and mask.shape == (len(values),)
        bad = np.flatnonzero(mask != want)
        assert bad.size == 0, (pattern, nocase, [(int(c), values[c], int(mask[c])) for c in bad[:5]])
        assert n == int(want.sum()), (pattern, nocase)
        dev, n_dev = d.like(pattern, nocase=nocase, out="device")
        assert np.array_equal(dev.to_host(), want) and n_dev == n and dev.n == len(values), (pattern, nocase)
        hits = int(want.sum())
    return hits


def edge_values():
    """per length the filler alone, and the filler with 'aXc' / 'AxC' ending at, straddling (one and two bytes over) and starting on every
    8-byte word edge — every second one a 16-byte edge — that the length reaches"""
    out = []
    for n in LENGTHS:
        out.append(b"." * n)
        for e in range(0, n + 8, 8):
            for at in (e - 3, e - 2, e - 1, e):
                if at >= 0 and at + 3 <= n:
                    for text in (b"aXc", b"AxC"):
                        out.append(b"." * at + text + b"." * (n - at - 3))
        if n >= 3:
            out.append(b"." * (n - 3) + b"aXc")               # the text at the value's end, whatever the length
    return list(dict.fromkeys(out))


EDGE_PATTERNS = ["%aXc%", "%a_c%", "%a_c", "a_c%", "%aXc", "%axc%", "%c", "_%", "%_a_c_%", "%.aXc.%", "%a%c%", "%.a_c", "a%", "%c.", "%\\.aXc%", "%aXc........%", "........%",
                 "%........a_c%", "_______a%", "_______________a%", "%a_c_______", "%a_c_______________", "%AXC%", "%ax_%"]


@pytest.fixture(scope="module")
def edges(engine):
    values = edge_values()
    d = held(engine, values)
    yield d, values
    d.close()


@pytest.mark.parametrize("pattern", EDGE_PATTERNS)
def test_value_lengths_and_the_text_at_every_word_edge(edges, pattern):
    d, values = edges
    assert {len(v) for v in values} == set(LENGTHS)
    hits = check(d, values, pattern)
    assert 0 < hits < len(values), pattern


def test_one_character_across_a_word_edge_and_malformed_bytes(engine):
    chars = ["é".encode(), "日".encode(), "😀".encode()]
    assert [len(c) for c in chars] == [2, 3, 4]
    values = []
    for ch in chars:
        for edge in (8, 16, 32):
            for at in range(edge - len(ch), edge + 1):       # from "ends at the edge" to "starts on it"
                values += [b"." * at + ch + b"z", b"." * at + ch + ch + b"z", b"q" * at + ch]
    values += like_ref.MALFORMED + [b"." * 7 + m for m in like_ref.MALFORMED] + [b"." * 15 + m for m in like_ref.MALFORMED]
    values = list(dict.fromkeys(values))
    d = held(engine, values)
    patterns = [b"%._z", b"%.__z", b"%_z", b"%__z", b"_______z", b"________z", b"%q_", b"%._", b"_%_z", b"_" * 9 + b"%", b"_" * 17, b"_" * 33,
                "%é_z".encode(), "%_日z".encode(), "%.😀%".encode(), b"%\xe6_", b"%_\xa5%"] + like_ref.MALFORMED_PATTERNS
    some = 0
    for p in patterns:
        some += check(d, values, p) > 0
    assert some >= len(patterns) - 4
    d.close()


def test_the_pattern_table(engine):
    values = list(dict.fromkeys([v.encode() for _, v, _, _ in like_ref.TABLE] + like_ref.MALFORMED))
    d = held(engine, values)
    for p in dict.fromkeys(p for p, _, _, _ in like_ref.TABLE):
        check(d, values, p)
    for p, v, want_nocase, want_case in like_ref.TABLE:       # and the table's own verdicts, straight from the device
        c = values.index(v.encode())
        assert d.like(p, nocase=True)[0][c] == want_nocase and d.like(p, nocase=False)[0][c] == want_case, (p, v)
    mask, n = d.like("")                                        # an empty pattern selects "" alone
    assert n == 1 and mask[values.index(b"")] == 1
    d.close()


def test_the_longest_pattern_is_accepted_and_one_byte_more_refused(engine):
    values = [b"a" * 1022, b"a" * 1021, b"xA" + b"a" * 1021 + b"yz", b"x" * 1024, b"x" * 1023, b"x" * 1025, b"ab" * 511, b"", b"\\" * 512]
    d = held(engine, values)
    for p in (b"%" + b"a" * 1022 + b"%", b"_" * 1024, b"%" + b"_" * 1023, b"%" * 1024, b"\\" * 1024, b"a_" * 512, b"%" + b"a_" * 511 + b"%"):
        assert len(p) == 1024
        check(d, values, p)
    assert d.like(b"%" + b"a" * 1022 + b"%", nocase=True)[1] == 2 and d.like(b"_" * 1024)[1] == 1
    for out in ("host", "device"):
        with pytest.raises(TadError) as ei:
            d.like(b"%" * 1025, out=out)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "at most 1024 bytes" in ei.value.message
    check(d, values, b"%a%")                                    # the next call is served
    d.close()


@pytest.mark.parametrize("count", COUNTS)
def test_value_counts(engine, count):
    rng = np.random.default_rng(count)
    values = [b"pod-%d-" % i + rng.integers(97, 123, int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for i in range(count)]
    d = held(engine, values)
    for p in ("%", "pod-_-%", "pod-%5-%", "%a%z%", "%-", "p%", "POD%q_"):
        check(d, values, p)
    assert d.like("pod-%")[1] == count and d.like("%")[1] == count and d.like("")[1] == 0
    d.close()


def test_one_value_more_than_the_grid_has_lanes(engine):
    """the launcher caps the grid at kSdLikeMaxBlocks workgroups of kSdBlock lanes: with one value more the stride loop runs"""
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    cap = int(re.search(r"kSdLikeMaxBlocks = (\d+);", open(os.path.join(csrc, "tad_internal.h")).read()).group(1))
    unit = open(os.path.join(csrc, "tad_strdict.hip")).read()
    block = int(re.search(r"kSdBlock = (\d+);", unit).group(1))
    assert "b < kSdLikeMaxBlocks ? b : kSdLikeMaxBlocks" in unit and "gridDim.x * kSdBlock" in unit[unit.index("void k_sd_like("):unit.index("void k_sd_export_lens(")]
    count = cap * block + 1
    assert count <= 1 << 20                                     # (keeps the case at seconds)
    values = [b"%07d" % i for i in range(count)]
    d = held(engine, values)
    hits = check(d, values, "%12_4%")
    assert hits > 1000
    mask = d.like("%_%")[0]                                     # the last value, the lone one of the second round, is answered
    assert mask.all() and d.like("%07d" % (count - 1))[0][count - 1] == 1
    d.close()


def test_after_growth_and_after_compact(engine):
    rng = np.random.default_rng(5)
    label = lambda i: b'{"app":"%s","test_key":"v%d","n":"%d"}' % ((b"web", b"Db", b"test-key")[i % 3], i % 7, i)
    first, second = [label(i) for i in range(300)], [label(i) + b"x" * int(rng.integers(1, 200)) for i in range(300, 5000)]
    d = engine.string_dict(1, 1)
    patterns = ('%"test_key":"v3"%', "%test\\_key%", "%app%d_\"%", "{%}", '%"n":"4__"%')
    d.encode(column(first, 64))
    before = d.nbytes()
    for p in patterns:
        check(d, first, p)
    d.encode(column(second, 64))
    assert d.nbytes() > before and d.num_values() == 5000      # table, records and arena grew
    values = first + second
    for p in patterns:
        check(d, values, p)
    keep = (np.arange(5000) % 3 != 2).astype(np.uint8)
    remap, _ = d.compact(keep)
    survivors = [v for v, k in zip(values, keep) if k]
    assert d.num_values() == len(survivors) and remap.max() == len(survivors) - 1
    for p in patterns:
        assert check(d, survivors, p) > 0
    d.close()


def test_refusals_leave_the_mask_untouched(engine):
    values = [b"alpha", b"beta", b"gamma_1", b""]
    d = held(engine, values)
    lib, inv = engine._lib, capi.TAD_ERR_INVALID_ARGUMENT
    pat = (C.c_ubyte * 2)(*b"%a")
    pp = C.cast(pat, C.c_void_p)
    mask = np.full(8, 0x5A, dtype=np.uint8)
    n = C.c_uint64(77)
    host, dev = capi.TAD_MEM_HOST, capi.TAD_MEM_DEVICE
    for stale in (3, 5, 0):                                     # a stale mask_len, in either direction
        assert lib.tad_strdict_like(engine._h, d._h, pp, 2, 0, mask.ctypes.data, stale, host, C.byref(n)) == inv
        assert b"mask has %d entries, the dictionary holds 4 values" % stale in lib.tad_last_error(engine._h)
    for flags in (2, 3, 0x80000000):                            # an unknown flag bit
        assert lib.tad_strdict_like(engine._h, d._h, pp, 2, flags, mask.ctypes.data, 4, host, C.byref(n)) == inv
    assert lib.tad_strdict_like(engine._h, d._h, pp, 2, 0, mask.ctypes.data, 4, 7, C.byref(n)) == inv           # a memory kind there is not
    assert lib.tad_strdict_like(engine._h, None, pp, 2, 0, mask.ctypes.data, 4, host, C.byref(n)) == inv        # no dictionary
    assert lib.tad_strdict_like(engine._h, d._h, None, 2, 0, mask.ctypes.data, 4, host, C.byref(n)) == inv      # a length without a pattern
    assert lib.tad_strdict_like(engine._h, d._h, pp, 2, 0, None, 4, dev, C.byref(n)) == inv                     # a length without a mask
    assert (mask == 0x5A).all() and n.value == 77
    assert lib.tad_strdict_like(engine._h, d._h, pp, 2, 0, mask.ctypes.data, 4, host, None) == capi.TAD_OK      # n_matched may be NULL
    assert mask[:4].tolist() == [1, 1, 0, 0] and (mask[4:] == 0x5A).all()
    with pytest.raises(TadError):
        d.like("%", out="pinned")
    check(d, values, "%a")
    d.close()
    empty = engine.string_dict(1, 1)                            # an empty dictionary: TAD_OK, nothing to write
    for out in ("host", "device"):
        mask, hit = empty.like("%", out=out)
        assert hit == 0 and (mask.n if out == "device" else mask.size) == 0
    empty.close()


def test_a_wildcard_free_pattern_between_percent_signs_is_the_contains_operation(engine):
    rng = np.random.default_rng(11)
    apps = (b"web", b"Web-Front", b"db", b"cache", b"DNS")
    values = [b'{"app":"%s","tier":"t%d","n":"%d","hash":"%s"}' % (apps[i % 5], i % 4, i, rng.integers(97, 123, int(rng.integers(0, 30)), dtype=np.uint8).tobytes()) for i in range(700)]
    d = held(engine, values)
    for text in ("web", "WEB", '"app":"db"', "t3", "front", "", "{", "}", "no-such-label", '"tier":"t1","n":"', "w", "E"):
        want, n_want = d.match(capi.TAD_STR_CONTAINS_NOCASE, text)
        got, n_got = d.like("%" + text + "%", nocase=True)
        assert np.array_equal(got, want) and n_got == n_want, text
        check(d, values, "%" + text + "%")
    d.close()
