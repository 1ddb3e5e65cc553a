"""Host: tests/slot_model.py — the restated hashes, the linear-probing model and the searchers the slot-table GPU tests rest on.  Every
searcher's result is checked again with tb_hash / se_hash called directly on the keys it returned."""
import numpy as np
import pytest

import slot_model as sm
from slot_model import Strings, Tuples
from job_helpers import hash8

U64 = np.uint64


def test_se_hash_of_8_byte_strings_is_hash8_of_test_gpu_strdict():
    words = np.arange(3000, dtype=U64) * U64(0x0101010101010101) + U64(0x2020202020202020)
    want = hash8(words)
    assert [sm.se_hash(int(w).to_bytes(8, "little")) for w in words[:300]] == [int(h) for h in want[:300]]
    assert np.array_equal(sm.se_hash_words(8, [words]), want)


def test_the_vectorised_hashes_equal_the_scalar_ones_at_every_length_and_width():
    for length in list(range(0, 35)) + [63, 64, 65]:
        for chunk in range(max((length + 7) // 8, 1)):
            fam = Strings(length, chunk, start=3)
            n = min(40, fam.room())
            keys = [fam.key(i) for i in range(n)]
            assert all(len(k) == length for k in keys) and len(set(keys)) == n
            assert fam.hashes(0, n).tolist() == [sm.se_hash(k) for k in keys], (length, chunk)
    for n_cols in range(1, 9):
        for side in (0, 1):
            for vary in (0, -1):
                fam = Tuples(n_cols, side, vary, start=-7)
                keys = [fam.key(i) for i in range(20)]
                assert all(k[0] == side and len(k[1]) == n_cols for k in keys) and len(set(keys)) == 20
                assert fam.hashes(0, 20).tolist() == [sm.hash_of(k) for k in keys]
    # the side and the column order are part of the hash; a column more is another hash
    assert sm.hash_of((0, (1, 2))) != sm.hash_of((1, (1, 2))) != sm.hash_of((0, (2, 1))) != sm.hash_of((0, (1, 2, 0)))
    # mix is the splitmix64 finaliser: its value at 1 is the published one
    assert int(sm.mix(np.array([1], dtype=U64))[0]) == 0x5692161D100B05E5


def test_occupied_does_not_depend_on_the_order_and_place_agrees_with_it():
    rng = np.random.default_rng(1)
    h = Tuples(3).hashes(0, 20).tolist() + [sm.hash_of(k) for k in sm.with_home(Tuples(1), 64, 60, 8, 12)]      # with a crowd at the table's end: 32 keys in 64 slots
    assert len(h) == 32
    occ = sm.occupied(64, h)
    for seed in range(3):
        p = [h[i] for i in rng.permutation(len(h))]
        assert sm.occupied(64, p) == occ
        slots = sm.place(64, p)
        assert set(slots) == occ and len(set(slots)) == len(p)
        for s, x, n in zip(slots, p, sm.passed(64, p)):
            assert (sm.home(x, 64) + n) % 64 == s


def test_passes_ends_at_an_empty_slot_at_load_one_half():
    h = Tuples(2).hashes(0, 512).tolist()
    occ = sm.occupied(1024, h)
    assert len(occ) == 512
    for x in h + Tuples(2).hashes(512, 700).tolist():
        walk = sm.passes(1024, occ, x)
        assert all(s in occ for s in walk) and len(walk) < 512
        nxt = (sm.home(x, 1024) + len(walk)) % 1024
        assert nxt not in occ and walk == [(sm.home(x, 1024) + k) % 1024 for k in range(len(walk))]


PAIR_FAMILIES = [Tuples(1), Tuples(3), Tuples(8), Tuples(8, vary=0), Strings(8), Strings(24, 2)]


@pytest.mark.parametrize("fam", PAIR_FAMILIES, ids=repr)
@pytest.mark.parametrize("homes", ["equal", "within", "straddle"])
def test_fingerprint_pairs_keep_their_contract(fam, homes):
    pairs = sm.fingerprint_pairs(fam, slots=64, homes=homes)
    assert len(pairs) >= 4
    for x, y in pairs:
        hx, hy = sm.hash_of(x), sm.hash_of(y)
        assert x != y and sm.fingerprint(hx) == sm.fingerprint(hy) and hx != hy
        ax, ay = sm.home(hx, 64), sm.home(hy, 64)
        if homes == "equal":
            assert ax == ay
        elif homes == "within":
            assert 1 <= ax - ay <= 8
        else:
            assert ay >= 56 and ax < 8
    if isinstance(fam, Tuples):                       # the pair differs in the varied column alone
        v = fam.vary % fam.n_cols
        assert all(x[0] == y[0] and [c for c in range(fam.n_cols) if x[1][c] != y[1][c]] == [v] for x, y in pairs)
    elif fam.length == 24:                            # ... in the second 16-byte word alone
        assert all(x[:16] == y[:16] and x[16:] != y[16:] for x, y in pairs)


@pytest.mark.parametrize("fam,other", [(Tuples(1), Tuples(1, side=1)), (Tuples(3), Tuples(3, side=1)), (Tuples(8), Tuples(8, side=1)), (Strings(8), Strings(9))], ids=repr)
def test_cross_pairs_come_one_from_each_family(fam, other):
    pairs = sm.fingerprint_pairs(fam, other, count=2_000_000, slots=64, homes="equal")
    assert len(sm.fingerprint_pairs(fam, other, count=2_000_000)) > 500
    for x, y in pairs:
        hx, hy = sm.hash_of(x), sm.hash_of(y)
        assert sm.fingerprint(hx) == sm.fingerprint(hy) and sm.home(hx, 64) == sm.home(hy, 64)
        if isinstance(fam, Tuples):
            assert (x[0], y[0]) == (0, 1)
        else:
            assert (len(x), len(y)) == (8, 9)


@pytest.mark.parametrize("fam", [Tuples(1), Tuples(2, side=1), Tuples(7), Strings(7), Strings(9), Strings(17, 1), Strings(33, 3)], ids=repr)
@pytest.mark.parametrize("slots,first,width", [(64, 10, 3), (64, 59, 10), (256, 250, 4), (1024, 1012, 24), (1 << 20, (1 << 20) - 10, 32)])
def test_with_home_keeps_its_contract_and_a_window_past_the_end_wraps(fam, slots, first, width):
    count = 12
    keys = sm.with_home(fam, slots, first, width, count)
    more = sm.with_home(fam, slots, first, width, 5, skip=count)
    assert len(set(keys + more)) == count + 5
    homes = [sm.home(sm.hash_of(k), slots) for k in keys + more]
    assert all((a - first) % slots < width for a in homes)
    if first + width > slots:                         # the window reaches past the table's end: homes on both sides of it
        many = [sm.home(sm.hash_of(k), slots) for k in sm.with_home(fam, slots, first, width, 60)]
        assert any(a >= first for a in many) and any(a < (first + width) % slots for a in many)


def test_a_wrapping_cluster_visits_the_last_slot_and_then_slot_0():
    for fam in (Tuples(3), Strings(9)):
        keys = sm.with_home(fam, 64, 59, 5, 10)
        h = [sm.hash_of(k) for k in keys]
        assert sm.occupied(64, h) == {59, 60, 61, 62, 63, 0, 1, 2, 3, 4}
        walk = sm.passes(64, sm.occupied(64, h), h[0])
        at = walk.index(63)
        assert walk[at + 1] == 0 and walk[-1] == 4
        assert sum(s < sm.home(x, 64) for s, x in zip(sm.place(64, h), h)) == 5      # every home at the end, five keys behind the wrap
        c = sm.cover(fam, 64, 59, 10)
        assert sm.place(64, [sm.hash_of(k) for k in c]) == [59, 60, 61, 62, 63, 0, 1, 2, 3, 4]


def test_zero_extension_pairs_share_a_fingerprint_and_lengths_7_and_8_can_share_a_whole_hash():
    gaps = []
    for x, y in sm.zero_extension_pairs():
        assert x != y and x.rstrip(b"\0") == y.rstrip(b"\0") and len(x.rstrip(b"\0")) == 7 and max(len(x), len(y)) <= 16
        hx, hy = sm.se_hash(x), sm.se_hash(y)
        assert sm.fingerprint(hx) == sm.fingerprint(hy) and hx != hy
        gaps.append((sm.home(hx, 64) - sm.home(hy, 64)) % 64)
    assert gaps == [0, 19, 2]
    # the recipe finds them again around where they are (the whole range takes minutes)
    for i, a, b in sm._ZERO_EXTENSIONS:
        assert (i, min(a, b), max(a, b)) in sm.search_zero_extensions(i - 1000, i + 1000)
    # the length is xor-ed into the first chunk: a 7-byte string and the 8-byte one that differs from it by 7 ^ 8 in its first byte (and
    # ends in a zero byte) have ONE hash, all 64 bits.  The searchers walk consecutive counters, so clusters of mixed lengths hold such pairs.
    x = b"pod-7ab"
    y = bytes([x[0] ^ 7 ^ 8]) + x[1:] + b"\0"
    assert sm.se_hash(x) == sm.se_hash(y) and x != y[:7]


def test_spread_keys_stay_under_the_probe_limit_and_a_crowd_does_not():
    for fam in (Tuples(2), Strings(12, 1)):
        keys = sm.spread(fam, 256, 40)
        assert max(sm.passed(256, [sm.hash_of(k) for k in keys])) <= sm.MAX_PROBE
        crowd = sm.with_home(fam, 256, 250, 4, 40)
        assert max(sm.passed(256, [sm.hash_of(k) for k in crowd])) > sm.MAX_PROBE


def test_a_search_that_finds_nothing_raises():
    with pytest.raises(LookupError):
        sm.with_home(Strings(1), 1 << 20, 5, 1, 3)
    with pytest.raises(LookupError):
        sm.fingerprint_pairs(Tuples(1), count=1000)
