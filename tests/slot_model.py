"""A host model of the slot table of the four ingest encoders (theia_amd/csrc/tad_slots.h) and searchers that ENGINEER its hard cases.

The table is open addressing with linear probing: a key with hash h starts at slot h & (slots - 1), steps (s + 1) & (slots - 1), and its
slot holds the fingerprint h >> 32.  The two hashes are pure functions, restated here in numpy: tb_hash (tad_slots.h: key tuples, the side
is part of the tuple) and se_hash (tad_strbytes.h: byte strings in 8-byte little-endian chunks).  On top of them: where a set of keys
lands (occupied, place), what a probe walks over (passes), and searches over CONSECUTIVE candidates — no randomness anywhere — for keys
that share a fingerprint, keys whose home slots lie in a window (a window past the table's end wraps), keys that cover a run of slots.

Keys are what the tests hand to the engine: a tuple key is (side, (c0, .., c_{n-1})), a string key is bytes.  No engine call, no test in
this module; tests/test_slot_model.py checks it on the host, tests/test_gpu_slot_table.py pins it to the device's tables first and then
rests every engineered case on it.  A search that does not find what was asked raises LookupError: the test that needs the case fails."""
import functools
from dataclasses import dataclass

import numpy as np

U64 = np.uint64
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15          # kTupleSideB, and se_hash's start (xor the length)
STEP = 0x632BE59BD9B4E019            # added after every column (times c + 1) / every chunk
MAX_PROBE = 32                       # kKdMaxProbe, kSdMaxProbe, kFzMaxProbe, kSeMaxProbe
PAIR_CANDIDATES = 4_000_000          # N (N - 1) / 2 / 2^32 = 1862 expected same-fingerprint pairs
BLOCK = 1 << 18                      # with_home walks the candidates this many at a time


def mix(x):
    """fz_mix: the splitmix64 finaliser, on uint64 arrays"""
    with np.errstate(over="ignore"):
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def _mix_int(x):
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def tb_hash(cols, side=0):
    """the hash of key tuples: cols = 1 to 8 int64 arrays (or scalars) of one length, side 0 = a / 1 = b -> uint64 array"""
    assert 1 <= len(cols) <= 8
    with np.errstate(over="ignore"):
        h = U64(GOLDEN if side else 0)
        for c, x in enumerate(cols):
            x = np.atleast_1d(np.asarray(x, dtype=np.int64)).view(U64)
            h = mix(h ^ x) + U64((STEP * (c + 1)) & M64)
        return mix(np.atleast_1d(h))


def se_hash(b):
    """the hash of one byte string of any length -> int"""
    b = bytes(b)
    h = GOLDEN ^ len(b)
    for i in range(0, len(b), 8):
        h = (_mix_int(h ^ int.from_bytes(b[i:i + 8], "little")) + STEP) & M64
    return _mix_int(h)


def se_hash_words(length, words):
    """se_hash of many strings of one length: words[k] = chunk k of every string as little-endian uint64 (an array, or a scalar for a chunk
    all strings share), bytes beyond the length zero"""
    assert len(words) == (length + 7) // 8
    with np.errstate(over="ignore"):
        h = U64(GOLDEN ^ length)
        for w in words:
            h = mix(h ^ (w if isinstance(w, np.ndarray) else U64(w))) + U64(STEP)
        return mix(np.atleast_1d(h))


def hash_of(key):
    """a key as the tests hold it -> int"""
    if isinstance(key, (bytes, bytearray)):
        return se_hash(key)
    side, t = key
    return int(tb_hash([np.int64(v) for v in t], side)[0])


def home(h, slots):
    return h & (slots - 1) if isinstance(h, int) else h & U64(slots - 1)


def fingerprint(h):
    return h >> 32 if isinstance(h, int) else h >> U64(32)


# ---- the table ----
def place(slots, hashes_in_order):
    """each key's slot, for keys inserted one after the other into an empty table"""
    assert slots & (slots - 1) == 0 and len(hashes_in_order) < slots
    taken, out = set(), []
    for h in hashes_in_order:
        s = int(h) & (slots - 1)
        while s in taken:
            s = (s + 1) & (slots - 1)
        taken.add(s)
        out.append(s)
    return out


def occupied(slots, hashes):
    """the slots a linear-probing table holds after these keys, whatever the order they came in"""
    return set(place(slots, hashes))


def passes(slots, occ, h):
    """the slots a probe for h visits before the first empty one, in order"""
    out, s = [], int(h) & (slots - 1)
    while s in occ:
        out.append(s)
        s = (s + 1) & (slots - 1)
        assert len(out) < slots, "the table is full"
    return out


def passed(slots, hashes_in_order):
    """for keys inserted one after the other: how many slots each claim passed over"""
    return [(s - (int(h) & (slots - 1))) & (slots - 1) for s, h in zip(place(slots, hashes_in_order), hashes_in_order)]


def in_window(homes, slots, first, width):
    """homes in the cyclic window [first, first + width) of a table of `slots` slots (first + width > slots wraps)"""
    return ((homes - first) & (slots - 1)) < width if isinstance(homes, int) else ((homes - U64(first % slots)) & U64(slots - 1)) < U64(width)


# ---- candidate families: key i of a family, for i = 0, 1, 2 ...: consecutive integers in one column / one chunk ----
@dataclass(frozen=True)
class Tuples:
    """tuples of n_cols columns on one side: column `vary` = start + i, every other column c a constant (negative and large)"""
    n_cols: int
    side: int = 0
    vary: int = -1
    start: int = 0

    def _base(self, c):
        return (c + 1) * -(1 << 50) + 977 * c

    def room(self):
        return 1 << 40                                # candidates: more than any search walks

    def key(self, i):
        v = self.vary % self.n_cols
        return (self.side, tuple(self.start + int(i) if c == v else self._base(c) for c in range(self.n_cols)))

    def hashes(self, lo, hi):
        v = self.vary % self.n_cols
        return tb_hash([np.arange(self.start + lo, self.start + hi, dtype=np.int64) if c == v else np.int64(self._base(c)) for c in range(self.n_cols)], self.side)


@dataclass(frozen=True)
class Strings:
    """byte strings of one length: the 8-byte chunk `chunk` (or what the length leaves of it) = start + i little-endian, every other byte a
    fixed letter.  A length of 0 has one candidate, a width of w < 8 bytes 256^w."""
    length: int
    chunk: int = 0
    start: int = 0

    def width(self):
        return max(min(8, self.length - 8 * self.chunk), 0)

    def room(self):
        return 1 if self.length == 0 else (1 << (8 * self.width())) - self.start

    def _filler(self):
        return bytes(0x41 + (j % 26) for j in range(self.length))

    def key(self, i):
        if self.length == 0:
            return b""
        w, at = self.width(), 8 * self.chunk
        f = self._filler()
        return f[:at] + (self.start + int(i)).to_bytes(w, "little") + f[at + w:]

    def hashes(self, lo, hi):
        hi = min(hi, self.room())
        if self.length == 0:
            return np.array([se_hash(b"")] * max(hi - lo, 0), dtype=U64)
        f = self._filler() + b"\0" * 7
        words = [int.from_bytes(f[8 * k:8 * k + 8], "little") & ((1 << (8 * min(8, self.length - 8 * k))) - 1) for k in range((self.length + 7) // 8)]
        words[self.chunk] = np.arange(self.start + lo, self.start + hi, dtype=U64)
        return se_hash_words(self.length, words)


# ---- searchers ----
@functools.lru_cache(maxsize=None)
def _same_fingerprint(fam, other, count):
    """(i, j, hash of i, hash of j): every pair of candidates whose hashes share the high 32 bits — in both orders within one family; i
    from fam and j from other across two.  Only the pairs are kept: the hashes of all candidates (32 MB a family) go when this returns."""
    ha = fam.hashes(0, count)
    h = ha if other is None else np.concatenate([ha, other.hashes(0, count)])
    fp = h >> U64(32)
    order = np.argsort(fp, kind="stable")
    eq = np.flatnonzero(fp[order][1:] == fp[order][:-1])
    i, j = order[eq], order[eq + 1]                  # (i < j: the sort is stable)
    if other is not None:
        cross = (i < ha.size) & (j >= ha.size)
        i, j = i[cross], j[cross]
        return i, j - ha.size, h[i], h[j]
    i, j = np.concatenate([i, j]), np.concatenate([j, i])      # both orders: the conditions on the homes are not symmetric
    return i, j, h[i], h[j]


@functools.lru_cache(maxsize=None)
def fingerprint_pairs(fam, other=None, count=PAIR_CANDIDATES, slots=None, homes=None, d=8):
    """Pairs (x, y) of different keys with ONE fingerprint among the first `count` candidates of fam — or, with `other`, x from fam and y
    from other (another side, another length).  homes (with slots): a condition on the two home slots — "equal"; "within": y's home lies
    1 .. d slots in front of x's, without a wrap; "straddle": y's home in the last 8 slots, x's in the first 8.  -> a tuple of (x, y)."""
    i, j, hi, hj = _same_fingerprint(fam, other, count)
    if homes is not None:
        hx, hy = (hi & U64(slots - 1)).astype(np.int64), (hj & U64(slots - 1)).astype(np.int64)
        ok = {"equal": hx == hy, "within": (hx - hy >= 1) & (hx - hy <= d), "straddle": (hy >= slots - 8) & (hx < 8)}[homes]
        i, j = i[ok], j[ok]
    elif other is None:
        i, j = i[: i.size // 2], j[: j.size // 2]
    if i.size == 0:
        raise LookupError("no same-fingerprint pair (%s) among %d candidates of %r" % (homes, count, (fam, other)))
    return tuple((fam.key(a), (fam if other is None else other).key(b)) for a, b in zip(i.tolist(), j.tolist()))


@functools.lru_cache(maxsize=None)
def with_home(fam, slots, first, width, count, skip=0, limit=1 << 24):
    """`count` distinct keys of fam whose home slots lie in the cyclic window [first, first + width) of a table of `slots` slots, after
    passing over the first `skip` such candidates (so that two calls give disjoint keys)"""
    out, lo, room = [], 0, min(limit, fam.room())
    while len(out) < skip + count and lo < room:
        h = fam.hashes(lo, min(lo + BLOCK, room))
        out += (lo + np.flatnonzero(in_window(h & U64(slots - 1), slots, first, width))).tolist()
        lo += BLOCK
    if len(out) < skip + count:
        raise LookupError("%d keys of %r with a home in [%d, %d + %d) of %d slots: found %d" % (skip + count, fam, first, first, width, slots, len(out)))
    return tuple(fam.key(i) for i in out[skip:skip + count])


def cover(fam, slots, first, width, skip=0):
    """one key per home slot first, first + 1, .. (cyclic), in that order: inserted into a table where those slots are free, key k lands ON
    slot first + k"""
    return tuple(with_home(fam, slots, (first + k) & (slots - 1), 1, 1, skip)[0] for k in range(width))


# A string and the same string with zero bytes appended share the arena's padded 16 bytes, so only the LENGTH tells them apart once their
# fingerprints agree — and the length is hashed, so no search of a second finds such a pair.  The recipe (search_zero_extensions below): a
# content is seven bytes, counter i little-endian in five of them, then 01 01; it is hashed at the ten lengths 7 .. 16 (zero bytes appended:
# one chunk up to 8 bytes, a second chunk of zeros from 9 on); any two of the ten lengths whose hashes share the high 32 bits are a hit:
# 45 chances of 2^-32 a content.  i = 0 .. 1.2e9 gave these (80 s of the same loop in C, minutes in numpy); content i, the two lengths.
# Every use re-checks them with se_hash.
_ZERO_EXTENSIONS = ((1102599834, 7, 9), (218372030, 9, 8), (923342408, 9, 14))


def search_zero_extensions(lo, hi):
    """the recipe above over the contents lo .. hi - 1 -> [(i, shorter length, longer length)]; not called by any GPU test"""
    out = []
    for b in range(lo, hi, BLOCK):
        w = np.arange(b, min(b + BLOCK, hi), dtype=U64) | U64(0x0101 << 40)
        fp = [se_hash_words(n, [w] if n <= 8 else [w, 0]) >> U64(32) for n in range(7, 17)]
        for p in range(10):
            for q in range(p + 1, 10):
                out += [(b + int(k), 7 + p, 7 + q) for k in np.flatnonzero(fp[p] == fp[q])]
    return sorted(out)


def zero_extension_pairs():
    """(x, y): one content padded with zero bytes to two lengths, ONE fingerprint.  The first pair has one home slot in a 64-slot table; in
    the others y's home lies 19 and 2 slots in front of x's."""
    out = []
    for i, len_x, len_y in _ZERO_EXTENSIONS:
        c = (i | (0x0101 << 40)).to_bytes(7, "little")
        out.append((c + b"\0" * (len_x - 7), c + b"\0" * (len_y - 7)))
    return tuple(out)


def spread(fam, slots, count, skip=0):
    """`count` keys of fam no claim of which passes more than MAX_PROBE slots when they are inserted in order — simply the first candidates,
    checked"""
    keys = tuple(fam.key(i) for i in range(skip, skip + count))
    if max(passed(slots, [hash_of(k) for k in keys]), default=0) > MAX_PROBE:
        raise LookupError("the first %d candidates of %r cluster in %d slots" % (count, fam, slots))
    return keys
