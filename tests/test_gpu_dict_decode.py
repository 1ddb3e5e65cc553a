"""GPU: the decode side of the two dictionaries, bit for bit against plain Python.

tad_strdict_decode(codes) must give b"".join(vals[c] for c in codes) and the cumulative lengths, where vals is the list of strings in code
order (the dictionaries here are filled with StringDict.load: value i is string i); tad_keydict_gather(ids) must give tuples[id], where
tuples is the list in id order (KeyDict.load: key i is tuple i).  The cases sit on the copy kernel's edges (tad_strdict.hip, k_sd_decode):
a workgroup takes TILE consecutive rows and assembles their bytes in STAGE bytes of LDS, a row over LANE_MAX bytes of a staged tile is
assembled by a wavefront, a tile over STAGE bytes is copied string by string without the stage, and past MAX_BLOCKS workgroups the tiles
are taken in a grid stride.  Every case asserts its precondition from host-side numbers before the engine is asked."""
import ctypes as C

import numpy as np
import pytest

from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray

pytestmark = pytest.mark.gpu

TILE = 256             # kSdDecodeRows       rows per workgroup
STAGE = 16 * 1024      # kSdDecodeStage      bytes of a tile that is assembled in LDS
MAX_BLOCKS = 2048      # kSdDecodeMaxBlocks  workgroups before the grid strides
LANE_MAX = 128         # kSdDecodeLaneMax    bytes a row's own lane assembles
KD_BLOCK = 256         # kKdBlock            ids per workgroup of the gather
INV = capi.TAD_ERR_INVALID_ARGUMENT
HOST, DEV = capi.TAD_MEM_HOST, capi.TAD_MEM_DEVICE


# ------------------------------------------------------------------ the reference, and the ways to ask the engine
def reference(vals, codes):
    lens = np.fromiter((len(vals[c]) for c in codes), dtype=np.int64, count=len(codes))
    offsets = np.zeros(len(codes) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    return offsets, b"".join(vals[c] for c in codes)


def distinct(rng, lengths):
    """one string of random bytes per entry of lengths, all different (at most one entry may be 0)"""
    out, seen = [], set()
    for ln in lengths:
        s = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        while s in seen and ln:
            s = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        if s in seen:
            raise AssertionError("two empty strings")
        seen.add(s)
        out.append(s)
    return out


def loaded(engine, vals):
    d = engine.string_dict()
    d.load(list(vals))
    assert d.num_values() == len(vals)
    return d


def check(d, vals, codes, outs=("host", "device"), device_codes=False):
    codes = np.asarray(codes, dtype=np.int64)
    want_off, want = reference(vals, codes.tolist())
    arg = DeviceArray.from_host(d._engine, codes) if device_codes and codes.size else codes
    for out in outs:
        off, data = d.decode(arg, out=out)
        if out == "device":
            off, data = off.to_host(), data.to_host()
        assert np.array_equal(off, want_off), out
        assert data.tobytes() == want, out
    return want_off


# ------------------------------------------------------------------ decode: row counts, code orders, both outputs
@pytest.fixture(scope="module")
def short_vocab(engine):
    rng = np.random.default_rng(11)
    lengths = [0] + [int(x) for x in rng.integers(1, 41, 299)]
    vals = distinct(rng, lengths)
    d = loaded(engine, vals)
    yield d, vals
    d.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, MAX_BLOCKS * TILE + 300])
def test_row_counts_around_the_wavefront_the_tile_and_the_grid_cap(short_vocab, n):
    d, vals = short_vocab
    assert (n + TILE - 1) // TILE > MAX_BLOCKS or n <= 2 * TILE + 1       # the last count makes the grid stride
    codes = np.random.default_rng(n).integers(0, len(vals), n)
    check(d, vals, codes, device_codes=n % 2 == 1)


@pytest.mark.parametrize("order", ["identity", "reversed", "all equal", "random with repeats"])
def test_code_orders(short_vocab, order):
    d, vals = short_vocab
    K = len(vals)
    codes = {"identity": np.arange(K), "reversed": np.arange(K)[::-1].copy(), "all equal": np.full(700, 17),
             "random with repeats": np.random.default_rng(5).integers(0, K, 1000)}[order]
    check(d, vals, codes)
    if order == "identity":                                               # the whole vocabulary in order: what export gives
        off, data = d.export()
        want_off, want = reference(vals, list(range(K)))
        assert np.array_equal(off, want_off) and data.tobytes() == want


def test_take_gives_a_large_string_array(engine):
    pa = pytest.importorskip("pyarrow")
    vals = ["", "shop", "blog/web:http", "käse", "x" * 300]
    d = loaded(engine, [v.encode("utf-8") for v in vals])
    codes = [4, 0, 3, 3, 1, 2]
    got = d.take(codes)
    assert got.type == pa.large_string() and got.to_pylist() == [vals[c] for c in codes]
    assert d.values().to_pylist() == vals
    d.close()


# ------------------------------------------------------------------ decode: lengths
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 255, 256, STAGE - 1, STAGE, STAGE + 1]


@pytest.fixture(scope="module")
def length_vocab(engine):
    rng = np.random.default_rng(12)
    vals = distinct(rng, LENGTHS + [1 << 20])
    assert set(b"".join(vals[:-1])) == set(range(256))                   # every byte value, zeros among them, inside strings
    d = loaded(engine, vals)
    yield d, vals
    d.close()


@pytest.mark.parametrize("order", ["identity", "reversed", "each alone", "random with repeats"])
def test_every_length_edge(length_vocab, order):
    d, vals = length_vocab
    K = len(LENGTHS)                                                      # (the 1 MiB string has its own test)
    if order == "each alone":
        for c in range(K):
            check(d, vals, [c], outs=("device",))
        return
    codes = {"identity": np.arange(K), "reversed": np.arange(K)[::-1].copy(), "random with repeats": np.random.default_rng(6).integers(0, K, 300)}[order]
    check(d, vals, codes)


def test_one_string_of_a_mebibyte(length_vocab):
    d, vals = length_vocab
    big = len(vals) - 1
    assert len(vals[big]) == 1 << 20 > STAGE
    check(d, vals, [big])
    check(d, vals, [3, big, 5, big, 0], device_codes=True)


def test_the_arena_padding_does_not_leak_and_zero_bytes_survive(engine):
    """strings of zeros and of 0xFF beside each other, lengths 1 .. 40: a pad byte that leaked, or a zero that was dropped, moves every
    later byte"""
    vals = [bytes([0]) * k for k in range(1, 41)] + [bytes([255]) * k for k in range(1, 41)] + [bytes(range(256))]
    d = loaded(engine, vals)
    codes = np.random.default_rng(8).integers(0, len(vals), 2000)
    check(d, vals, codes)
    d.close()


# ------------------------------------------------------------------ decode: layout cases
def test_tile_starts_on_every_residue_mod_16(engine):
    rng = np.random.default_rng(13)
    vals = distinct(rng, [16] * 255 + [1])
    d = loaded(engine, vals)
    codes = np.tile(np.arange(TILE), 17)
    want_off = reference(vals, codes.tolist())[0]
    assert [int(want_off[TILE * t]) % 16 for t in range(17)] == [t % 16 for t in range(17)]      # tile t begins t bytes into a 16-byte word
    check(d, vals, codes)
    d.close()


def test_a_run_of_empty_strings_over_two_whole_tiles(short_vocab):
    d, vals = short_vocab
    assert vals[0] == b""
    codes = np.concatenate([np.arange(1, 101), np.zeros(3 * TILE, dtype=np.int64), np.arange(101, 151)])
    off = check(d, vals, codes)
    assert off[TILE] == off[3 * TILE] == off[100]                         # tiles 1 and 2 write no byte: the offsets are flat across them


def test_a_tile_of_exactly_the_stage_and_one_byte_over(engine):
    rng = np.random.default_rng(14)
    vals = distinct(rng, [64] * TILE + [65, 3])
    d = loaded(engine, vals)
    exact = np.arange(TILE)
    over = np.concatenate([np.arange(TILE - 1), [TILE]])
    codes = np.concatenate([exact, over, [TILE + 1] * 5, exact])
    off = reference(vals, codes.tolist())[0]
    assert off[TILE] - off[0] == STAGE and off[2 * TILE] - off[TILE] == STAGE + 1
    check(d, vals, codes)
    d.close()


@pytest.mark.parametrize("long_len", [LANE_MAX + 70, 5000, STAGE + 3000])
def test_a_long_string_first_last_and_alone_in_its_tile(engine, long_len):
    """LANE_MAX + 70 and 5000: a wavefront assembles the string in the stage; STAGE + 3000: its tile is not staged"""
    rng = np.random.default_rng(long_len)
    vals = distinct(rng, [long_len, 0] + [int(x) for x in rng.integers(1, 30, 60)])
    d = loaded(engine, vals)
    short = rng.integers(1, len(vals), TILE - 1)
    codes = np.concatenate([[0], short, short, [0], [0]])                  # first of tile 0, last of tile 1, alone in tile 2
    assert codes.size == 2 * TILE + 1 and codes[0] == codes[2 * TILE - 1] == codes[2 * TILE] == 0
    off = reference(vals, codes.tolist())[0]
    assert (off[TILE] - off[0] > STAGE) == (long_len > STAGE)
    check(d, vals, codes)
    d.close()


def test_device_data_at_every_byte_alignment_leaves_its_surroundings_alone(engine, short_vocab):
    d, vals = short_vocab
    rng = np.random.default_rng(15)
    longer = distinct(rng, [STAGE + 100])
    d2 = loaded(engine, list(vals) + longer)
    vals2 = list(vals) + longer
    codes = np.concatenate([rng.integers(0, len(vals), 2 * TILE + 40), [len(vals)], rng.integers(0, len(vals), 30)])
    want_off, want = reference(vals2, codes.tolist())
    total = len(want)
    dcodes = DeviceArray.from_host(engine, codes.astype(np.int64))
    doff = DeviceArray(engine, codes.size + 1, np.int64)
    room = (total + 64 + 7) // 8
    need = C.c_uint64()
    for shift in range(16):
        buf = DeviceArray.from_host(engine, np.full(room, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64))
        rc = engine._lib.tad_strdict_decode(engine._h, d2._h, dcodes.ptr, codes.size, DEV, doff.ptr, buf.ptr + 16 + shift, total, DEV, C.byref(need))
        assert rc == capi.TAD_OK and need.value == total, shift
        got = buf.to_host().view(np.uint8)
        assert got[16 + shift:16 + shift + total].tobytes() == want, shift
        assert (got[:16 + shift] == 0xEE).all() and (got[16 + shift + total:] == 0xEE).all(), shift
        assert np.array_equal(doff.to_host(), want_off)
        buf.free()
    d2.close()


# ------------------------------------------------------------------ decode: dictionary history
def test_after_growth_and_after_export_import(engine):
    rng = np.random.default_rng(16)
    d = engine.string_dict(1, 1)                                           # the smallest: table, records and arena all grow
    before = d.nbytes()
    vals = []
    for b in range(4):
        new = [b"batch%d-value%d-" % (b, i) + bytes(rng.integers(0, 256, int(rng.integers(0, 50)), dtype=np.uint8)) for i in range(500)]
        offsets = np.zeros(len(new) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in new], out=offsets[1:])
        codes, _, num_before = d.encode((offsets, np.frombuffer(b"".join(new), dtype=np.uint8)))
        assert num_before == len(vals) and np.array_equal(codes, np.arange(len(vals), len(vals) + len(new)))
        vals += new
        check(d, vals, rng.integers(0, len(vals), 700), outs=("host",))
    assert d.nbytes() > before
    d2 = engine.string_dict()
    d2.load(d.export())
    codes = rng.integers(0, len(vals), 1500)
    check(d, vals, codes)
    check(d2, vals, codes)
    d.close()
    d2.close()


# ------------------------------------------------------------------ decode: refusals
def raw_decode(engine, d, codes, offsets, data, cap, need, codes_mem=HOST, out_mem=HOST):
    ptr = lambda a: None if a is None else (a.ptr if isinstance(a, DeviceArray) else a.ctypes.data)
    return engine._lib.tad_strdict_decode(engine._h, d._h if d is not None else None, ptr(codes), 0 if codes is None else (codes.n if isinstance(codes, DeviceArray) else codes.size),
                                          codes_mem, ptr(offsets), ptr(data), cap, out_mem, C.byref(need) if need is not None else None)


@pytest.mark.parametrize("bad", [-1, "num_values", 1 << 40])
def test_a_code_outside_the_values_is_refused_with_nothing_written(engine, short_vocab, bad):
    d, vals = short_vocab
    bad = len(vals) if bad == "num_values" else bad
    assert capi.TAD_CODE_NONE == -1
    codes = np.random.default_rng(3).integers(0, len(vals), 600).astype(np.int64)
    codes[431] = bad
    offsets = np.full(601, -7, dtype=np.int64)
    data = np.full(40 * 600, 0xEE, dtype=np.uint8)
    need = C.c_uint64(99)
    assert raw_decode(engine, d, codes, offsets, data, data.size, need) == INV
    assert (offsets == -7).all() and (data == 0xEE).all()
    with pytest.raises(TadError) as ei:
        d.decode(DeviceArray.from_host(engine, codes), out="device")
    assert ei.value.code == INV


def test_data_cap_exact_one_under_and_the_size_query(engine, short_vocab):
    d, vals = short_vocab
    codes = np.random.default_rng(4).integers(0, len(vals), 900).astype(np.int64)
    want_off, want = reference(vals, codes.tolist())
    total = len(want)
    need = C.c_uint64(0)
    assert raw_decode(engine, d, codes, None, None, 0, need) == capi.TAD_OK and need.value == total          # the size query
    offsets = np.full(901, -7, dtype=np.int64)
    data = np.full(total, 0xEE, dtype=np.uint8)
    need = C.c_uint64(0)
    assert raw_decode(engine, d, codes, offsets, data, total - 1, need) == INV                                 # one under: nothing but *data_bytes
    assert need.value == total and (offsets == -7).all() and (data == 0xEE).all()
    assert raw_decode(engine, d, codes, offsets, data, total, None) == capi.TAD_OK                             # exact; data_bytes may be NULL
    assert np.array_equal(offsets, want_off) and data.tobytes() == want


def test_null_arguments_are_refused(engine, short_vocab):
    d, vals = short_vocab
    codes = np.zeros(4, dtype=np.int64)
    offsets, data, need = np.full(5, -7, dtype=np.int64), np.full(8, 0xEE, dtype=np.uint8), C.c_uint64(5)
    assert raw_decode(engine, None, codes, offsets, data, 8, need) == INV                                      # no dictionary
    assert raw_decode(engine, d, codes, None, data, 8, need) == INV                                            # data without offsets
    assert engine._lib.tad_strdict_decode(engine._h, d._h, None, 4, HOST, offsets.ctypes.data, data.ctypes.data, 8, HOST, C.byref(need)) == INV     # no codes
    assert raw_decode(engine, d, codes, offsets, data, 8, need, codes_mem=7) == INV
    assert need.value == 5 and (offsets == -7).all() and (data == 0xEE).all()
    assert raw_decode(engine, d, np.zeros(0, dtype=np.int64), offsets, None, 0, need) == capi.TAD_OK and need.value == 0 and offsets[0] == 0      # n == 0


def test_workspace_limit_refuses_a_host_call_before_anything_runs(engine, short_vocab):
    """a host call stages 8 B a code beside 12 B a row of lengths and offsets: 200 000 codes need 4 MB, the limit is 1 MiB"""
    _, vals = short_vocab
    small = TadEngine(device=engine.device, workspace_limit=1 << 20)
    try:
        d = loaded(small, vals)
        n = 200_000
        assert 20 * n > 1 << 20 > 20 * 1000
        check(d, vals, np.arange(1000) % len(vals), outs=("host",))
        with pytest.raises(TadError) as ei:
            d.decode(np.zeros(n, dtype=np.int64))
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        check(d, vals, np.arange(1000) % len(vals), outs=("host",))
        d.close()
    finally:
        small.close()


# ------------------------------------------------------------------ gather
def tuple_table(n_cols, K, seed):
    """K distinct tuples in id order, both sides, values over the whole int64 range"""
    rng = np.random.default_rng(seed)
    cols = [rng.integers(-2**62, 2**62, K) for _ in range(n_cols)]
    cols[0] = np.arange(K, dtype=np.int64) * 3 - 7                          # distinct whatever the rest holds
    side = (rng.random(K) < 0.4).astype(np.uint8)
    return cols, side


@pytest.fixture(scope="module", params=[1, 2, 3, 8])
def key_dict(engine, request):
    n_cols = request.param
    K = 700
    cols, side = tuple_table(n_cols, K, 20 + n_cols)
    assert side.any() and not side.all()
    kd = engine.key_dict(n_cols)
    kd.load(cols, side)
    assert kd.num_keys() == K
    yield kd, cols, side
    kd.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, KD_BLOCK - 1, KD_BLOCK, KD_BLOCK + 1, 2 * KD_BLOCK + 1])
def test_gather_row_counts_in_host_and_device_memory(engine, key_dict, n):
    kd, cols, side = key_dict
    ids = np.random.default_rng(n).integers(0, side.size, n).astype(np.uint64)
    for arg, out in ((ids, "host"), (ids, "device"), (DeviceArray.from_host(engine, ids) if n else ids, "host")):
        got, got_side = kd.gather(arg, out=out)
        if out == "device":
            got, got_side = [g.to_host() for g in got], got_side.to_host()
        assert len(got) == kd.n_cols
        for c in range(kd.n_cols):
            assert np.array_equal(got[c], cols[c][ids.astype(np.int64)]), (c, out)
        assert np.array_equal(got_side, side[ids.astype(np.int64)]), out


def test_gather_repeated_reversed_and_whole_range_equals_export(key_dict):
    kd, cols, side = key_dict
    K = side.size
    for ids in (np.full(300, 5), np.arange(K)[::-1].copy(), np.arange(K)):
        got, got_side = kd.gather(ids.astype(np.uint64))
        assert all(np.array_equal(got[c], cols[c][ids]) for c in range(kd.n_cols)) and np.array_equal(got_side, side[ids])
    exp_cols, exp_side = kd.export()
    got, got_side = kd.gather(np.arange(K, dtype=np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(got, exp_cols)) and np.array_equal(got_side, exp_side)


def test_gather_skips_a_null_column_and_a_null_side(engine, key_dict):
    kd, cols, side = key_dict
    ids = np.random.default_rng(9).integers(0, side.size, 500).astype(np.uint64)
    last = kd.n_cols - 1
    got, _ = kd.gather(ids, cols=[last])                                    # every other entry of the pointer array is NULL
    assert len(got) == 1 and np.array_equal(got[0], cols[last][ids.astype(np.int64)])
    for mem in (HOST, DEV):
        dids = DeviceArray.from_host(engine, ids)
        out = np.full(500, -7, dtype=np.int64)
        dout = DeviceArray.from_host(engine, out)
        ptrs = (C.c_void_p * kd.n_cols)(*([None] * last + [dout.ptr if mem == DEV else out.ctypes.data]))
        rc = engine._lib.tad_keydict_gather(engine._h, kd._h, dids.ptr if mem == DEV else ids.ctypes.data, 500, mem, ptrs, None)      # side NULL
        assert rc == capi.TAD_OK
        assert np.array_equal(dout.to_host() if mem == DEV else out, cols[last][ids.astype(np.int64)])


@pytest.mark.parametrize("bad", ["num_keys", "TAD_KEY_SKIP"])
def test_gather_refuses_an_id_that_is_no_key(engine, key_dict, bad):
    kd, cols, side = key_dict
    ids = np.arange(300, dtype=np.uint64)
    ids[123] = side.size if bad == "num_keys" else capi.TAD_KEY_SKIP
    for arg in (ids, DeviceArray.from_host(engine, ids)):
        with pytest.raises(TadError) as ei:
            kd.gather(arg)
        assert ei.value.code == INV
    got, _ = kd.gather(np.arange(300, dtype=np.uint64))                     # and the dictionary answers as before
    assert np.array_equal(got[0], cols[0][:300])


def test_gather_after_compact_gives_the_survivors(engine):
    cols, side = tuple_table(3, 600, 31)
    kd = engine.key_dict(3)
    kd.load(cols, side)
    live = np.random.default_rng(32).random(600) < 0.6
    remap = np.where(live, np.cumsum(live) - 1, -1).astype(np.int64).astype(np.uint64)
    m = int(live.sum())
    assert 0 < m < 600 and kd.compact(remap) == m
    got, got_side = kd.gather(np.arange(m, dtype=np.uint64))
    assert all(np.array_equal(got[c], cols[c][live]) for c in range(3)) and np.array_equal(got_side, side[live])
    with pytest.raises(TadError):
        kd.gather(np.asarray([m], dtype=np.uint64))
    kd.close()


def test_gather_of_encoded_batches_equals_export(engine):
    """a dictionary filled by encode, two-sided: whatever ids the batches got, gather over the whole range is export"""
    rng = np.random.default_rng(33)
    kd = engine.key_dict(2, 1)
    for _ in range(3):
        a = [rng.integers(0, 40, 2000), rng.integers(0, 30, 2000)]
        b = [rng.integers(0, 40, 2000), rng.integers(0, 30, 2000)]
        kd.encode(a, None, b, None)
    K = kd.num_keys()
    assert K > 1000
    exp_cols, exp_side = kd.export()
    assert exp_side.any() and not exp_side.all()
    perm = rng.permutation(K).astype(np.uint64)
    got, got_side = kd.gather(perm)
    assert all(np.array_equal(got[c], exp_cols[c][perm.astype(np.int64)]) for c in range(2)) and np.array_equal(got_side, exp_side[perm.astype(np.int64)])
    kd.close()
