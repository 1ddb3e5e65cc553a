"""GPU: the persistent string dictionary (tad_strdict, include/tad.h) — the strings of an Arrow column -> codes that stay the same from batch
to batch, new codes in order of first appearance.  The oracle is a Python dict over the rows of every batch in order; the stability case is
also held against tad_encode_strings over the concatenation of the batches, restricted to each batch.  Every dictionary starts at the
smallest table and arena (expected_values=1, expected_bytes=1) unless a case says otherwise, so that the growth of the table, the records and
the arena is on the path of nearly every case.  After every refusal the dictionary is compared with a snapshot (num_values, the full export)."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import STAGE, column, device_column, exported, hash8, host

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
ROWS = (1, 63, 64, 65, 255, 256, 257, 511, 513, 4097)


class Oracle:
    """bytes -> code, codes in order of first appearance over the rows of every batch"""

    def __init__(self):
        self.ids = {}

    def run(self, strings, insert=True):
        before = len(self.ids)
        codes, first = np.empty(len(strings), dtype=np.int64), []
        for i, s in enumerate(strings):
            c = self.ids.get(s)
            if c is None:
                if insert:
                    c = self.ids[s] = len(self.ids)
                    first.append(i)
                else:
                    c = -1
            codes[i] = c
        return codes, np.array(first, dtype=np.uint64), before

    def values(self):
        return sorted(self.ids, key=self.ids.get)


def strdict_snapshot(d):
    return d.num_values(), exported(d)


def assert_strdict_unchanged(d, snap):
    assert (d.num_values(), exported(d)) == snap


def assert_batch(got, want, what=""):
    codes, first, before = got
    wcodes, wfirst, wbefore = want
    assert before == wbefore, (what, before, wbefore)
    assert np.array_equal(host(codes), wcodes), what
    assert np.array_equal(host(first), wfirst), what


def special_strings(rng):
    """every length of LENGTHS twice, pairs that differ only in the first or only in the last byte, every prefix of one 40-byte string, and
    strings that differ only in trailing zero bytes"""
    out = []
    for n in LENGTHS:
        for _ in range(2):
            out.append(rng.integers(1, 255, n, dtype=np.uint8).tobytes())
        if n:
            s = bytearray(out[-1])
            s[0] ^= 0x20
            out.append(bytes(s))
            s = bytearray(out[-2])
            s[-1] ^= 0x01
            out.append(bytes(s))
    long = rng.integers(97, 123, 40, dtype=np.uint8).tobytes()
    out += [long[:k] for k in range(41)]
    out += [b"a", b"a\0", b"a\0\0", b"\0", b"\0\0"]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("rows", ROWS)
def test_row_counts_and_string_lengths(engine, rows):
    rng = np.random.default_rng(rows)
    vocab = special_strings(rng)
    d, orc = engine.string_dict(1, 1), Oracle()
    for b in range(2):
        pick = rng.integers(0, len(vocab) if b else len(vocab) // 2, rows)
        batch = [vocab[i] for i in pick]
        assert_batch(d.encode(column(batch)), orc.run(batch), (rows, b))
        assert exported(d) == orc.values()
    look = [vocab[i] for i in rng.integers(0, len(vocab), rows)] + [b"never seen", b"a\0\0\0"]
    assert np.array_equal(d.lookup(column(look)), orc.run(look, insert=False)[0])
    assert exported(d) == orc.values()
    d.close()


def test_every_special_string_is_its_own_value(engine):
    """first-byte and last-byte neighbours, the prefixes of one string and "a" / "a\\0" / "a\\0\\0": zero-masked word loads must not make any
    two of them equal — in one batch (de-duplicated among the misses) and against the arena (the second batch)"""
    vocab = special_strings(np.random.default_rng(7))
    d = engine.string_dict(1, 1)
    codes, first, before = d.encode(column(vocab))
    assert before == 0 and np.array_equal(codes, np.arange(len(vocab))) and np.array_equal(first, np.arange(len(vocab), dtype=np.uint64))
    codes, first, before = d.encode(column(vocab[::-1]))
    assert before == len(vocab) and first.size == 0 and np.array_equal(codes, np.arange(len(vocab))[::-1])
    assert exported(d) == vocab
    d.close()


@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("shift", range(16))
def test_device_slices_at_every_byte_offset_with_nulls_that_own_bytes(engine, shift, bits):
    rng = np.random.default_rng(100 + shift)
    vocab = special_strings(rng)
    d, orc = engine.string_dict(1, 1), Oracle()
    for b in range(2):
        batch = [vocab[i] for i in rng.integers(0, len(vocab), 300)]
        valid = rng.random(300) > 0.2
        valid[:2] = (True, False)
        seen = [s if v else b"" for s, v in zip(batch, valid)]          # a null row that still owns bytes encodes like ""
        got = d.encode(device_column(engine, batch, bits, shift, valid, validity_offset=3 + b), out="device")
        assert isinstance(got[0], DeviceArray)
        assert_batch(got, orc.run(seen), (shift, bits, b))
    assert exported(d) == orc.values()
    d.close()


@pytest.mark.parametrize("span", (STAGE - 1, STAGE, STAGE + 1))
def test_the_staging_edge(engine, span):
    """the first block's 256 rows span exactly `span` bytes measured from the 16-byte aligned start the kernel stages from"""
    rng = np.random.default_rng(span)
    shift = 5
    total = span - shift
    lens = [total // 256] * 255
    lens.append(total - sum(lens))
    first_block = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    tail = [rng.integers(97, 123, 12, dtype=np.uint8).tobytes() for _ in range(100)] + first_block[:50]
    batch = first_block + tail
    col = device_column(engine, batch, 32, shift)
    off = col[0].to_host()
    start = col[1].ptr + int(off[0])
    assert (col[1].ptr + int(off[256])) - (start & ~15) == span                # the span the kernel compares with its stage
    d, orc = engine.string_dict(1, 1), Oracle()
    assert_batch(d.encode(col, out="device"), orc.run(batch), "cold")
    assert_batch(d.encode(col, out="device"), orc.run(batch), "warm")       # every string known: the probe compares with the arena
    assert exported(d) == orc.values()
    d.close()


def test_one_long_string_among_short_ones(engine):
    rng = np.random.default_rng(3)
    long = rng.integers(0, 256, 30000, dtype=np.uint8).tobytes()
    batch = [b"x%d" % (i % 40) for i in range(300)]
    batch[17] = long
    batch[290] = long[:-1] + b"!"
    batch[299] = long
    d, orc = engine.string_dict(1, 1), Oracle()
    for mem in ("host", "device", "host"):
        col = column(batch) if mem == "host" else device_column(engine, batch, 32, 9)
        assert_batch(d.encode(col, out=mem), orc.run(batch), mem)
    assert exported(d) == orc.values()
    d.close()


@pytest.mark.parametrize("memory", ("host", "device"))
def test_codes_are_stable_over_six_overlapping_batches(engine, memory):
    rng = np.random.default_rng(11)
    names = [b"pod-%x-%d" % (int(rng.integers(1 << 30)), i) for i in range(900)] + [b""]
    d, orc = engine.string_dict(1, 1), Oracle()
    so_far = []
    for b in range(6):
        lo = b * 120
        batch = [names[i] for i in rng.integers(max(lo - 200, 0), lo + 300, 700)]
        col = column(batch) if memory == "host" else device_column(engine, batch, 32, b)
        got = d.encode(col, out=memory)
        assert_batch(got, orc.run(batch), b)
        so_far += batch
        whole, _ = engine.encode_strings(column(so_far))                         # one call on the concatenation of batches 1 .. b
        assert np.array_equal(host(got[0]), whole[len(so_far) - len(batch):]), b
    assert exported(d) == orc.values()
    # a cap of 0 and a cap of 1 cap only the list
    for cap in (0, 1):
        batch = [b"capped-%d-%d" % (cap, i % 5) for i in range(40)] + [names[3]]
        col = column(batch) if memory == "host" else device_column(engine, batch)
        codes, first, before = d.encode(col, out=memory, max_new=cap)
        wcodes, wfirst, wbefore = orc.run(batch)
        assert before == wbefore and np.array_equal(host(codes), wcodes) and np.array_equal(host(first), wfirst[:cap])
        assert d.num_values() == wbefore + 5
    assert exported(d) == orc.values()
    d.close()


def test_growth_at_the_first_tables_load_limit(engine):
    d, orc = engine.string_dict(1, 1), Oracle()
    size0 = d.nbytes()
    assert size0 == 64 * 8 + 32 * 16 + 16                                       # the smallest table, records and arena
    first = [b"v%02d" % i for i in range(32)]
    assert_batch(d.encode(column(first)), orc.run(first))
    assert exported(d) == orc.values()
    more = first[::-1] + [b"v32"]
    assert_batch(d.encode(column(more)), orc.run(more))
    assert exported(d) == orc.values() and d.num_values() == 33 and d.nbytes() > size0
    d.close()


def test_growth_through_70000_values(engine):
    d, orc = engine.string_dict(1, 1), Oracle()
    for b in range(7):
        batch = [b"flow-key-%07d" % i for i in range(b * 10000, (b + 1) * 10000)]
        if b:
            batch[5] = b"flow-key-%07d" % 17                                     # one known string among the new ones
        codes, first, before = d.encode(column(batch))
        wcodes, wfirst, wbefore = orc.run(batch)
        assert before == wbefore and np.array_equal(codes, wcodes) and np.array_equal(first, wfirst)
        assert exported(d) == orc.values()
    assert d.num_values() == 70000 - 6
    d.close()


def test_a_megabyte_of_strings_into_a_one_byte_arena(engine):
    rng = np.random.default_rng(5)
    batch = [rng.integers(0, 256, 1024 + (i % 7), dtype=np.uint8).tobytes() for i in range(1000)]
    d, orc = engine.string_dict(1, 1), Oracle()
    assert_batch(d.encode(column(batch)), orc.run(batch))
    assert exported(d) == orc.values()
    assert d.nbytes() >= sum(len(s) for s in batch)
    d.close()


def test_many_rows_of_three_values(engine):
    rng = np.random.default_rng(6)
    vals = [b"", b"kube-system", b"default"]
    batch = [vals[i] for i in rng.integers(0, 3, 100000)]
    d, orc = engine.string_dict(1, 1), Oracle()
    for _ in range(2):
        assert_batch(d.encode(column(batch)), orc.run(batch))
    assert exported(d) == orc.values()
    d.close()


def test_two_strings_with_one_fingerprint_are_two_values(engine):
    """Among 4e5 8-byte strings the expected number of pairs whose hashes share the high 32 bits — the slot's fingerprint — is
    N (N - 1) / 2 / 2^32 = 18.6; the probability of none is e^-18.6.  Such a pair is told apart by the bytes alone.  Whether the two probe
    sequences meet in the 64-slot table is left to chance here; the case where they do is built in tests/test_gpu_slot_table.py."""
    words = np.arange(400000, dtype=np.uint64) * np.uint64(0x0101010101010101) + np.uint64(0x2020202020202020)
    fp = hash8(words) >> np.uint64(32)
    order = np.argsort(fp, kind="stable")
    same = np.flatnonzero(fp[order][1:] == fp[order][:-1])
    assert same.size > 0
    a, b = (words[order[same[0]]].tobytes(), words[order[same[0] + 1]].tobytes())
    assert a != b and len(a) == 8
    d = engine.string_dict(1, 1)
    codes, first, before = d.encode(column([a, b, a, b]))
    assert np.array_equal(codes, [0, 1, 0, 1]) and np.array_equal(first, [0, 1])      # apart among the misses of one batch
    codes, first, _ = d.encode(column([b, a, b"other888"]))
    assert np.array_equal(codes, [1, 0, 2]) and np.array_equal(first, [2])            # and against the arena
    d2 = engine.string_dict(1, 1)
    assert np.array_equal(d2.encode(column([a]))[0], [0])
    assert np.array_equal(d2.lookup(column([b, a])), [-1, 0])                         # the fingerprint alone is not a hit
    assert np.array_equal(d2.encode(column([b]))[0], [1])
    assert exported(d2) == [a, b] and exported(d) == [a, b, b"other888"]
    mask, hit = d.match(capi.TAD_STR_EQUAL, b)
    assert hit == 1 and np.array_equal(mask, [0, 1, 0])
    d.close()
    d2.close()


def test_lookup_and_an_empty_batch_change_nothing(engine):
    d = engine.string_dict(1, 1)
    assert d.encode(column([]))[2] == 0 and d.num_values() == 0
    assert np.array_equal(d.lookup(column([b"x", b""])), [-1, -1])
    d.encode(column([b"x", b"y"]))
    snap = strdict_snapshot(d)
    assert np.array_equal(d.lookup(column([b"y", b"z", b"x", b""])), [1, -1, 0, -1])
    assert np.array_equal(d.lookup(device_column(engine, [b"y", b"z", b"x"], 64, 3), out="device").to_host(), [1, -1, 0])
    codes, first, before = d.encode(column([]))
    assert codes.size == 0 and first.size == 0 and before == 2
    assert_strdict_unchanged(d, snap)
    d.close()


def test_pyarrow_columns_with_nulls_and_slices(engine):
    pa = pytest.importorskip("pyarrow")
    vals = ["ns-%d" % (i % 9) if i % 5 else None for i in range(200)]
    d, orc = engine.string_dict(1, 1), Oracle()
    for arr in (pa.array(vals, type=pa.string()), pa.array(vals, type=pa.large_string()).slice(37, 120), pa.chunked_array([pa.array(vals[:50]), pa.array(vals[50:])])):
        want = [(v or "").encode() for v in arr.to_pylist()]
        assert_batch(d.encode(arr), orc.run(want))
    assert d.values().to_pylist() == [v.decode() for v in orc.values()]
    assert d.values(2, 3).to_pylist() == [v.decode() for v in orc.values()[2:5]]
    d.close()


def raw_encode(engine, d, off, data, data_bytes=None, bits=32):
    n = off.size - 1
    codes, first = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint64)
    sc = capi.StringColumn(n_rows=n, offsets=off.ctypes.data, offset_bits=bits, data=data.ctypes.data, data_bytes=data.size if data_bytes is None else data_bytes,
                           validity=None, validity_offset=0, memory=capi.TAD_MEM_HOST)
    before, after = capi.u64(99), capi.u64(99)
    rc = engine._lib.tad_strdict_encode(engine._h, d._h, C.byref(sc), codes.ctypes.data, first.ctypes.data, n, C.byref(before), C.byref(after))
    return rc, after.value


def test_malformed_offsets_are_refused_before_the_dictionary_is_touched(engine):
    d = engine.string_dict(1, 1)
    d.encode(column([b"held", b"too"]))
    snap = strdict_snapshot(d)
    strings = [b"new-%d" % i for i in range(600)]
    off, data = column(strings)
    bad = off.copy()
    bad[500] = bad[499] - 2                                                      # decreases, behind 499 rows of new strings
    assert raw_encode(engine, d, bad, data)[0] == capi.TAD_ERR_INVALID_ARGUMENT
    assert_strdict_unchanged(d, snap)
    bad = off.copy()
    bad[-1] += 40                                                                # points beyond data_bytes
    assert raw_encode(engine, d, bad, data)[0] == capi.TAD_ERR_INVALID_ARGUMENT
    assert_strdict_unchanged(d, snap)
    assert raw_encode(engine, d, off, data, data_bytes=data.size - 1)[0] == capi.TAD_ERR_INVALID_ARGUMENT
    assert_strdict_unchanged(d, snap)
    assert raw_encode(engine, d, off.astype(np.int64), data, bits=16)[0] == capi.TAD_ERR_INVALID_ARGUMENT
    assert_strdict_unchanged(d, snap)
    with pytest.raises(TadError) as ei:
        d.lookup((bad, data))
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
    rc, after = raw_encode(engine, d, off, data)                                 # the same batch, passed properly
    assert rc == capi.TAD_OK and after == 602 and d.num_values() == 602
    d.close()


def test_workspace_limit_refuses_a_big_batch_and_leaves_the_dictionary_unchanged(engine):
    """Scratch (include/tad.h): n bytes of miss flags; a batch with unknown strings adds tad_encode_strings' scratch, whose table alone is
    8 bytes x (the power of two >= 2 n).  With a limit of 1 MiB a device batch of 1000 rows passes; one of 100 000 unknown strings needs
    more than 16 x 100 000 bytes for that table and is refused — after the probe, before the dictionary is touched.  The same 100 000
    rows with KNOWN strings need the flags only, and pass."""
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    try:
        d = small.string_dict(1, 1)
        first = [b"k%d" % i for i in range(1000)]
        codes, _, before = d.encode(device_column(small, first), out="device")
        assert before == 0 and np.array_equal(codes.to_host(), np.arange(1000)) and d.num_values() == 1000
        snap = strdict_snapshot(d)
        big = device_column(small, [b"n%d" % i for i in range(100_000)])
        with pytest.raises(TadError) as ei:
            d.encode(big, out="device")
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        assert_strdict_unchanged(d, snap)
        known = device_column(small, [b"k%d" % (i % 1000) for i in range(100_000)])
        codes, fr, before = d.encode(known, out="device")
        assert before == 1000 and fr.n == 0 and np.array_equal(codes.to_host(), np.arange(100_000) % 1000)
        assert_strdict_unchanged(d, snap)
        d.close()
    finally:
        small.close()


def test_export_ranges_the_size_query_and_a_small_buffer(engine):
    vocab = special_strings(np.random.default_rng(8))
    d = engine.string_dict(1, 1)
    d.encode(column(vocab))
    K = len(vocab)
    for first, n in ((0, K), (0, 0), (K, 0), (3, 1), (K - 5, 5), (10, 77)):
        assert exported(d, first, n) == vocab[first:first + n], (first, n)
    lib, need = engine._lib, capi.u64(0)
    assert lib.tad_strdict_export(engine._h, d._h, 4, 30, None, None, 0, C.byref(need)) == capi.TAD_OK
    want = sum(len(s) for s in vocab[4:34])
    assert need.value == want
    off, data = np.full(31, -7, np.int64), np.full(want, 0xEE, np.uint8)
    need = capi.u64(0)
    assert lib.tad_strdict_export(engine._h, d._h, 4, 30, off.ctypes.data, data.ctypes.data, want - 1, C.byref(need)) == capi.TAD_ERR_INVALID_ARGUMENT
    assert need.value == want and (off == -7).all() and (data == 0xEE).all()          # nothing written but the size
    assert lib.tad_strdict_export(engine._h, d._h, 4, 30, off.ctypes.data, data.ctypes.data, want, C.byref(need)) == capi.TAD_OK
    assert off[0] == 0 and off[-1] == want and data.tobytes() == b"".join(vocab[4:34])
    for first, n in ((K + 1, 0), (0, K + 1), (K - 1, 2)):
        assert lib.tad_strdict_export(engine._h, d._h, first, n, None, None, 0, C.byref(need)) == capi.TAD_ERR_INVALID_ARGUMENT
    d.close()


def test_import_restores_the_codes_and_refuses_what_it_must(engine):
    vocab = special_strings(np.random.default_rng(9))
    d = engine.string_dict(1, 1)
    d.encode(column(vocab))
    saved = d.export()
    r = engine.string_dict(1, 1)
    r.load(saved)
    assert exported(r) == vocab and r.num_values() == len(vocab)
    probe = vocab[::-3] + [b"new after the restart"]
    codes, first, before = r.encode(column(probe))
    want = np.array([vocab.index(s) for s in probe[:-1]] + [len(vocab)])
    assert before == len(vocab) and np.array_equal(codes, want) and np.array_equal(first, [len(probe) - 1])
    snap = strdict_snapshot(r)
    with pytest.raises(TadError) as ei:                                          # it already holds values
        r.load(saved)
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
    assert_strdict_unchanged(r, snap)
    e = engine.string_dict(1, 1)
    for bad in ([b"a", b"b", b"a"], [b"", b"x", b""], [b"a\0", b"a", b"a\0"]):       # two strings are equal
        with pytest.raises(TadError) as ei:
            e.load(bad)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and e.num_values() == 0 and exported(e) == []
    off, data = column([b"ab", b"cd", b"ef"], 64)
    for bad in (off + 1, np.array([0, 4, 2, 6], np.int64)):                      # do not start at 0 / decrease
        with pytest.raises(TadError) as ei:
            e.load((bad, np.concatenate([data, data])))
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and e.num_values() == 0
    e.load(["x", "", "y"])                                                      # still empty and usable
    assert exported(e) == [b"x", b"", b"y"]
    assert np.array_equal(e.encode(column([b"", b"y", b"x"]))[0], [1, 2, 0])
    for x in (d, r, e):
        x.close()


FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def match_oracle(values, op, pat):
    if op == capi.TAD_STR_EQUAL:
        return np.array([v == pat for v in values], dtype=np.uint8)
    p = pat.translate(FOLD)
    return np.array([p in v.translate(FOLD) for v in values], dtype=np.uint8)


def test_match_equal_and_contains_without_case(engine):
    rng = np.random.default_rng(12)
    labels = ['{"app":"Web-%d","tier":"FrontEnd"}' % i for i in range(40)] + ['{"app":"db","Tier":"backend-%d"}' % i for i in range(40)]
    vocab = [s.encode() for s in labels] + ["Éclair-É".encode(), "éclair-é".encode(), b"", b"a", b"A", b"aa", b"aA\0a", b"\xc0\xe0", b"\xe0\xc0", b"[@`{"]
    vocab += [rng.integers(65, 123, n, dtype=np.uint8).tobytes() for n in (7, 8, 9, 15, 16, 17, 31, 32, 33, 200, 1030)]
    vocab += [b"x" * 1023 + b"Needle", b"needle" + b"y" * 1100, b"nEEdl" * 30 + b"needle"]
    vocab = list(dict.fromkeys(vocab))
    d = engine.string_dict(1, 1)
    d.encode(column(vocab))
    pats = [b"", b"a", b"A", b"web-1", b"WEB-1", b'"tier":"frontend"', b"Tier", "É".encode(), "é".encode(), b"\xe0", b"\xc0\xe0", b"@", b"`", b"[", b"{",
            b"needle", b"NEEDLE" + b"Y" * 1018, b"x" * 1024, vocab[3], vocab[-6], vocab[-6][3:], vocab[-5][100:140], vocab[-7][1:16], vocab[-8][2:19],
            b"a\0a", b"A\0", b"zzzz-nowhere"]
    for op in (capi.TAD_STR_EQUAL, capi.TAD_STR_CONTAINS_NOCASE):
        for pat in pats:
            assert len(pat) <= 1024
            want = match_oracle(vocab, op, pat)
            mask, hit = d.match(op, pat)
            assert np.array_equal(mask, want) and hit == int(want.sum()), (op, pat[:40])
    assert d.match(capi.TAD_STR_EQUAL, b"")[1] == 1 and d.match(capi.TAD_STR_CONTAINS_NOCASE, b"")[1] == len(vocab)
    # a device mask is what KeyDict.select takes
    mask, hit = d.match(capi.TAD_STR_CONTAINS_NOCASE, "frontend", out="device")
    assert isinstance(mask, DeviceArray) and mask.n == len(vocab) and np.array_equal(mask.to_host(), match_oracle(vocab, 1, b"frontend")) and hit == 40
    kd = engine.key_dict(1, 1)
    kd.encode([np.arange(len(vocab), dtype=np.int64)[::-1].copy()])
    keep, n_sel = kd.select([(0, mask)], out="device")
    assert n_sel == 40 and np.array_equal(keep.to_host(), match_oracle(vocab, 1, b"frontend")[::-1])
    kd.close()
    # refusals: a pattern over 1024 bytes, an unknown op, a stale mask length — nothing is written
    snap = strdict_snapshot(d)
    for op, pat in ((capi.TAD_STR_EQUAL, b"p" * 1025), (2, b"p"), (-1, b"p")):
        with pytest.raises(TadError) as ei:
            d.match(op, pat)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT
    stale = np.full(len(vocab) + 1, 9, np.uint8)
    hit = capi.u64(77)
    p = (C.c_ubyte * 1)(97)
    for n in (len(vocab) - 1, len(vocab) + 1, 0):
        rc = engine._lib.tad_strdict_match(engine._h, d._h, 0, C.cast(p, C.c_void_p), 1, stale.ctypes.data, n, capi.TAD_MEM_HOST, C.byref(hit))
        assert rc == capi.TAD_ERR_INVALID_ARGUMENT and (stale == 9).all() and hit.value == 77
    assert_strdict_unchanged(d, snap)
    empty = engine.string_dict(1, 1)
    mask, hit = empty.match(capi.TAD_STR_CONTAINS_NOCASE, b"")
    assert mask.size == 0 and hit == 0
    empty.close()
    d.close()


def test_many_values_match_like_the_oracle(engine):
    """more values than one workgroup, every alignment of a hit inside the 8-byte words of a value"""
    vocab = [b"-" * (i % 23) + (b"PoD" if i % 3 else b"pad") + b"+" * (i % 19) + b"%d" % i for i in range(3000)]
    d = engine.string_dict(1, 1)
    d.encode(column(vocab))
    for pat in (b"pod", b"d+", b"-p", b"29"):
        want = match_oracle(vocab, 1, pat)
        mask, hit = d.match(capi.TAD_STR_CONTAINS_NOCASE, pat)
        assert np.array_equal(mask, want) and hit == int(want.sum()), pat
    d.close()
