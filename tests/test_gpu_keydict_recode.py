"""GPU: tad_keydict_mark_codes and tad_keydict_recode (include/tad.h, TAD_FEATURE_STRING_RETIRE).  The references are numpy's isin over
the tuples' columns and a plain list of tuples; every comparison is exact.  Dictionaries are filled with KeyDict.load, which takes the
tuples and their sides as they are; column 0 of every tuple is unique, so the tuples are.  Key counts sit on the wavefront (64) and the
workgroup (256) of the kernels and past the scan-free grid of one launch; the 65-key refusals put the offender into the second wavefront."""
import numpy as np
import pytest

from theia_amd import TadEngine, TadError, _capi as capi
from theia_amd.engine import DeviceArray
from job_helpers import SKIP, column

pytestmark = pytest.mark.gpu

KEYS = [1, 63, 64, 65, 256, 257, 2049]


def tuples(K, n_cols, seed, V=None, two_sided=True):
    """K distinct tuples over codes [0, V) and their sides"""
    rng = np.random.default_rng(seed)
    V = V or K + 5
    cols = [rng.permutation(V)[:K].astype(np.int64)] + [rng.integers(0, V, K).astype(np.int64) for _ in range(n_cols - 1)]
    side = (rng.integers(0, 2, K) if two_sided else np.zeros(K)).astype(np.uint8)
    return cols, side, V


def loaded(engine, cols, side):
    d = engine.key_dict(len(cols), 1)
    d.load(cols, side)
    return d


def dev_bytes(engine, a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    base = DeviceArray.from_host(engine, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8), dtype=np.uint64))
    return base.view(0, a.size, np.uint8)


def recode_snapshot(d):
    cols, side = d.export()
    return [c.tolist() for c in cols], side.tolist(), d.num_keys(), d.nbytes()


def lookup_ids(d, cols, side):
    """the ids of the tuples (cols, side): every tuple is offered on both sides, each side kept where it is the tuple's"""
    a, b = d.lookup(cols, side == 0, cols, side == 1)
    return np.where(side == 0, a, b)


# ---- mark_codes ----

@pytest.mark.parametrize("K", KEYS)
@pytest.mark.parametrize("n_cols", [1, 2, 8])
def test_mark_codes_is_isin_over_the_column_on_both_sides(engine, K, n_cols):
    cols, side, V = tuples(K, n_cols, 10 * K + n_cols)
    d = loaded(engine, cols, side)
    for col in sorted({0, n_cols - 1, n_cols // 2}):
        want = np.isin(np.arange(V), cols[col]).astype(np.uint8)
        used, n = d.used_codes(col, V, out="host")
        assert np.array_equal(used, want) and n == int(want.sum())
        used, n = d.used_codes(col, V)                                     # device memory
        assert isinstance(used, DeviceArray) and np.array_equal(used.to_host(), want) and n == int(want.sum())
    # the mask may be longer than the codes in use: the rest is zero
    used, n = d.used_codes(0, V + 100, out="host")
    assert np.array_equal(used, np.isin(np.arange(V + 100), cols[0])) and n == K
    d.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_accumulate_ors_two_columns_into_one_mask(engine, memory):
    cols, side, V = tuples(300, 3, 77)
    d = loaded(engine, cols, side)
    used, n0 = d.used_codes(0, V, out=memory)
    both, n = d.used_codes(2, V, into=used, out=memory)
    want = np.isin(np.arange(V), np.concatenate([cols[0], cols[2]])).astype(np.uint8)
    got = both.to_host() if memory == "device" else both
    assert np.array_equal(got, want) and n == int(want.sum()) and n0 == 300
    # what the mask held stays: ones outside every column are counted too
    pre = np.zeros(V, dtype=np.uint8)
    free = np.flatnonzero(want == 0)
    pre[free[:3]] = 1
    arg = dev_bytes(engine, pre) if memory == "device" else pre.copy()
    got, n = d.used_codes(1, V, into=arg, out=memory)
    want1 = np.isin(np.arange(V), cols[1]).astype(np.uint8) | pre
    assert np.array_equal(got.to_host() if memory == "device" else got, want1) and n == int(want1.sum())
    d.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_a_code_at_the_masks_end_passes_and_one_beyond_is_refused(engine, memory):
    K = 65
    cols, side, V = tuples(K, 2, 5)
    cols[1][64] = V + 6                                                      # the largest code, held by a key of the second wavefront
    d = loaded(engine, cols, side)
    used, n = d.used_codes(1, V + 7, out=memory)                             # used_len - 1
    got = used.to_host() if memory == "device" else used
    assert got[V + 6] == 1 and np.array_equal(got, np.isin(np.arange(V + 7), cols[1]))
    snap = recode_snapshot(d)
    with pytest.raises(TadError) as ei:
        d.used_codes(1, V + 6, out=memory)                                   # used_len: outside
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "outside" in ei.value.message
    with pytest.raises(TadError):
        d.used_codes(1, 0, out=memory)
    for bad_col in (-1, 2):
        with pytest.raises(TadError) as ei:
            d.used_codes(bad_col, V + 7, out=memory)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "column" in ei.value.message
    assert recode_snapshot(d) == snap                                               # read-only throughout
    d.close()


@pytest.mark.parametrize("shift,extra", [(1, 0), (3, 5), (7, 1), (0, 7), (5, 3)])
def test_a_device_mask_at_any_byte_alignment_and_length_is_counted_byte_for_byte(engine, shift, extra):
    """the count reads the aligned body of the mask eight bytes at a time and the bytes at its two ends singly"""
    cols, side, _ = tuples(257, 2, 61, V=2048 + extra)
    V = 2048 + extra
    d = loaded(engine, cols, side)
    pre = (np.random.default_rng(shift).integers(0, 9, V) == 0).astype(np.uint8) * np.uint8(0x80)      # any non-zero byte counts, bit 7 alone too
    pad = np.concatenate([np.full(shift, 0xEE, np.uint8), pre, np.full(-(shift + V) % 8 + 8, 0xEE, np.uint8)])
    base = DeviceArray.from_host(engine, np.frombuffer(pad.tobytes(), dtype=np.uint64))
    got, n = d.used_codes(1, V, into=base.view(shift, V, np.uint8))
    want = np.where(np.isin(np.arange(V), cols[1]), 1, pre).astype(np.uint8)
    assert np.array_equal(got.to_host(), want) and n == int((want != 0).sum())
    whole = base.to_host().view(np.uint8)
    assert (whole[:shift] == 0xEE).all() and (whole[shift + V:] == 0xEE).all()                           # nothing outside the mask is written
    short, n = d.used_codes(0, 2048 + extra, out="device")
    assert n == 257
    tiny = engine.key_dict(1, 1)
    tiny.load([np.array([2, 0, 4], dtype=np.int64)], None)
    for L in (5, 7, 8, 9, 15, 16, 17):
        used, n = tiny.used_codes(0, L)
        assert n == 3 and np.array_equal(used.to_host(), np.isin(np.arange(L), [0, 2, 4]))
    tiny.close()
    d.close()


def test_an_empty_dictionary_marks_nothing(engine):
    d = engine.key_dict(2, 1)
    used, n = d.used_codes(1, 10, out="host")
    assert n == 0 and not used.any()
    used, n = d.used_codes(0, 10)
    assert n == 0 and not used.to_host().any()
    pre = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    got, n = d.used_codes(0, 5, into=pre.copy(), out="host")                # accumulate: what it held
    assert np.array_equal(got, pre) and n == 3
    assert d.used_codes(0, 0, out="host")[1] == 0
    d.close()


# ---- recode ----

def check_recode(engine, K, n_cols, terms, seed, memory="host"):
    """terms: {col: kind}; kind "perm" a permutation of the codes, "up" strictly increasing, "id" the identity"""
    cols, side, V = tuples(K, n_cols, seed)
    rng = np.random.default_rng(seed + 1)
    remaps = {c: {"perm": rng.permutation(V), "up": 2 * np.arange(V) + 1, "id": np.arange(V)}[kind].astype(np.int64) for c, kind in terms.items()}
    new_cols = [remaps[c][cols[c]] if c in remaps else cols[c].copy() for c in range(n_cols)]
    d = loaded(engine, cols, side)
    nbytes = d.nbytes()
    keep = [DeviceArray.from_host(engine, r) for r in remaps.values()] if memory == "device" else None
    arg = dict(zip(remaps, keep)) if memory == "device" else remaps
    assert d.recode(arg) == K
    assert d.num_keys() == K and d.nbytes() == nbytes                       # fresh arrays of the current sizes
    got_cols, got_side = d.export()
    assert all(np.array_equal(g, w) for g, w in zip(got_cols, new_cols)) and np.array_equal(got_side, side)     # ids unchanged, the new codes
    ids = np.random.default_rng(seed + 2).permutation(K).astype(np.uint64)
    g_cols, g_side = d.gather(ids)
    assert all(np.array_equal(g, w[ids]) for g, w in zip(g_cols, new_cols)) and np.array_equal(g_side, side[ids])
    assert np.array_equal(lookup_ids(d, new_cols, side), np.arange(K, dtype=np.uint64))          # new tuples -> old ids
    old_tuples = set(zip(side.tolist(), *[c.tolist() for c in cols]))
    new_tuples = set(zip(side.tolist(), *[c.tolist() for c in new_cols]))
    gone = np.array([t not in new_tuples for t in zip(side.tolist(), *[c.tolist() for c in cols])])
    if new_tuples != old_tuples:
        assert (lookup_ids(d, cols, side)[gone] == SKIP).all() and gone.any()      # a tuple in old codes is no longer held
    # a later encode of tuples in new codes: the known ones keep their ids, new ones are appended
    extra = [np.concatenate([nc[:5], np.full(3, 10 * V + 7 + i, dtype=np.int64)]) for i, nc in enumerate(new_cols)]
    a, b, first, before = d.encode(extra, np.concatenate([side[:5] == 0, np.ones(3, bool)]), extra, np.concatenate([side[:5] == 1, np.zeros(3, bool)]))
    assert before == K and np.array_equal(np.where(np.concatenate([side[:5], np.zeros(3, np.uint8)]) == 0, a, b),
                                          np.concatenate([np.arange(min(5, K)), [K, K, K]]).astype(np.uint64)[:extra[0].size])
    d.close()


@pytest.mark.parametrize("K", KEYS)
def test_recode_one_term_with_a_permutation(engine, K):
    check_recode(engine, K, 2, {0: "perm"}, 100 + K)


@pytest.mark.parametrize("n_cols,terms", [(1, {0: "up"}), (2, {1: "perm"}), (3, {0: "perm", 2: "up"}), (8, {7: "perm", 0: "up"}), (8, {3: "perm"}),
                                          (2, {0: "id", 1: "perm"})])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_recode_one_and_two_terms_host_and_device_remaps(engine, n_cols, terms, memory):
    check_recode(engine, 257, n_cols, terms, 7 * n_cols + len(terms), memory)


@pytest.mark.parametrize("how", ["identity", "no-terms", "identity-on-the-values-held"])
def test_the_identity_leaves_the_dictionary_untouched(engine, how):
    cols, side, V = tuples(300, 2, 31)
    d = loaded(engine, cols, side)
    snap = recode_snapshot(d)
    if how == "identity":
        assert d.recode({0: np.arange(V), 1: np.arange(V)}) == 300
    elif how == "no-terms":
        assert d.recode({}) == 300
    else:                                                  # entries no key holds may say anything
        r = np.arange(V, dtype=np.int64)
        r[~np.isin(np.arange(V), cols[1])] = -1
        assert d.recode({1: r}) == 300
    assert recode_snapshot(d) == snap
    assert np.array_equal(lookup_ids(d, cols, side), np.arange(300, dtype=np.uint64))
    d.close()
    e = engine.key_dict(2, 1)                              # an empty dictionary
    assert e.recode({0: np.arange(3)}) == 0 and e.num_keys() == 0
    e.close()


@pytest.mark.parametrize("what", ["none", "outside", "negative-value", "twice", "collision", "bad-column"])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_refusals_leave_the_dictionary_unchanged(engine, what, memory):
    K = 65                                                 # key 64 is the offender: the second wavefront
    cols, side, V = tuples(K, 2, 900, two_sided=False)
    remap = np.random.default_rng(4).permutation(V).astype(np.int64)
    col1 = np.arange(V, dtype=np.int64)
    if what == "none":
        remap[cols[0][64]] = capi.TAD_CODE_NONE            # a key still uses a retired string
    elif what == "outside":
        cols[0][64] = V + 3                                # beyond the remap's V entries
    elif what == "negative-value":
        cols[0][64] = -5
    elif what == "collision":
        cols[1][64], cols[1][3] = 9, 9                     # keys 3 and 64 differ in column 0 only ...
        remap[cols[0][64]] = remap[cols[0][3]]             # ... and no longer after it
    d = loaded(engine, cols, side)
    snap = recode_snapshot(d)
    terms = [(0, remap), (1, col1)]
    if what == "twice":
        terms = [(0, remap), (0, remap)]
    elif what == "bad-column":
        terms = [(2, remap)]
    if memory == "device":
        terms = [(c, DeviceArray.from_host(engine, r)) for c, r in terms]
    with pytest.raises(TadError) as ei:
        d.recode(terms)
    assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and "unchanged" in ei.value.message
    assert recode_snapshot(d) == snap
    assert np.array_equal(lookup_ids(d, cols, side), np.arange(K, dtype=np.uint64))
    a, _, first, before = d.encode([np.array([cols[0][0], 10 ** 6]), np.array([cols[1][0], 1])])      # and it still takes keys
    assert before == K and np.array_equal(a, [0, K])
    d.close()


def test_a_remap_of_a_small_workspace_limit_engine_is_refused_whole():
    """a host remap is staged in job-context workspace: 200 000 entries of 8 bytes do not fit 1 MiB, the same remap in device memory needs none"""
    small = TadEngine(device=0, workspace_limit=1 << 20)
    try:
        cols, side, V = tuples(500, 1, 3, V=200_000)
        d = loaded(small, cols, side)
        snap = recode_snapshot(d)
        remap = np.random.default_rng(8).permutation(V).astype(np.int64)
        with pytest.raises(TadError) as ei:
            d.recode({0: remap})
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE and recode_snapshot(d) == snap
        with pytest.raises(TadError) as ei:
            d.used_codes(0, 2_000_000, out="host")
        assert ei.value.code == capi.TAD_ERR_GRID_TOO_LARGE
        assert d.recode({0: DeviceArray.from_host(small, remap)}) == 500
        assert np.array_equal(d.export()[0][0], remap[cols[0]])
        d.close()
    finally:
        small.close()


# ---- the chain ----


def decoded(sd, codes):
    off, data = sd.decode(codes)
    raw = data.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(off.size - 1)]


@pytest.mark.parametrize("memory", ["device", "host"])
def test_the_chain_mark_compact_recode_keeps_every_keys_strings(engine, memory):
    """3000 keys over a vocabulary of 500 strings of which 37 are still used: afterwards the vocabulary holds the 37, in their old order,
    and every key decodes to the strings it decoded to before"""
    rng = np.random.default_rng(2024)
    names = [b"pod-%03d-%s" % (i, b"xyzxyzxyzxyzxyzxyzxyz"[:i % 20]) for i in range(500)]
    sd = engine.string_dict(1, 1)
    assert np.array_equal(sd.encode(column(names, 64))[0], np.arange(500))
    live = np.sort(rng.choice(500, 37, replace=False))
    cols = [live[rng.integers(0, 37, 3000)].astype(np.int64), np.arange(3000, dtype=np.int64)]
    cols[0][:37] = live                                    # every one of the 37 is used
    side = rng.integers(0, 2, 3000).astype(np.uint8)
    kd = loaded(engine, cols, side)
    ids = np.arange(3000, dtype=np.uint64)
    before = decoded(sd, kd.gather(ids)[0][0])
    assert before == [names[c] for c in cols[0]]
    used, n_used = kd.used_codes(0, sd.num_values(), out=memory)
    assert n_used == 37
    remap, st = sd.compact(used, out=memory)
    assert (st["values_before"], st["values_after"]) == (500, 37)
    assert kd.recode({0: remap}) == 3000
    g_cols, g_side = kd.gather(ids)
    assert decoded(sd, g_cols[0]) == before and np.array_equal(g_cols[1], cols[1]) and np.array_equal(g_side, side)
    assert sd.num_values() == 37 and decoded(sd, np.arange(37)) == [names[c] for c in live]
    assert g_cols[0].max() == 36 and np.array_equal(np.unique(g_cols[0]), np.arange(37))
    # a second round with nothing to retire is the identity everywhere
    snap = recode_snapshot(kd)
    used, n_used = kd.used_codes(0, 37, out=memory)
    remap, st = sd.compact(used, out=memory)
    assert n_used == 37 and st["values_after"] == 37 and np.array_equal(remap.to_host() if memory == "device" else remap, np.arange(37))
    kd.recode({0: remap})
    assert recode_snapshot(kd) == snap
    kd.close()
    sd.close()
