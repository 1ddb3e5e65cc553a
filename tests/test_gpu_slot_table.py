"""GPU: the slot table of the four ingest encoders (theia_amd/csrc/tad_slots.h) on ENGINEERED hash collisions — the branches random input
almost never reaches: a fingerprint match that is not equality and is met on the probe sequence, a probe that wraps from the last slot to
slot 0, a cluster longer than the probe limit at low load, the atomic min deep inside a cluster, the duplicate check of an import across
a wrap, a rehash into a smaller table.  tests/slot_model.py restates the two hashes and linear probing and finds the keys by search on the
host; every test asserts from that model that its case IS the case (which slots are taken, what a probe walks over, how far a claim
passes) before the engine is asked.  The reference is plain Python — a dict of (side, tuple) or of bytes over the rows in order: ids by
first appearance over [side a ++ side b], first rows, dictionary exports as lists, TAD_KEY_SKIP / -1 for a miss — and every comparison
is exact.

THE PINS come first (test_pin_*): a wrong restatement of a hash would make every engineered case vacuous.  A dictionary of 256 slots is
given, one call each, keys whose homes the model puts in a window 4 slots wide; KD_FLAG_CLUSTER / SD_FLAG_CLUSTER (a claim that passed
more than 32 slots) must double the table at exactly the call the model names — nbytes() rises by the 256 new slots' bytes there and at no
call before it — and must not for a control of as many keys the model calls spread.  tad_factorize and tad_encode_strings hash with the same
two functions (tb_hash_col / fz_mix in k_fz_insert, se_hash's loop in k_se_insert), so the pins hold for them: they expose no table size, and
their probe-limit retries (test_*_probe_limit_*) are reached by construction, resting on these pins.

Two things the searches bring along.  se_hash xors the length into the first chunk, so a 7-byte string and the 8-byte one that differs from it
by 7 ^ 8 in the first byte and ends in a zero byte share ALL 64 bits of the hash; the mixed-length clusters here are found over consecutive
counters and hold such pairs (home and fingerprint equal, lengths different): more of case 1 in every cluster test.  And a string and its own
zero-extension, which only the length check can tell apart in the zero-padded arena, cannot be found in a second: three such pairs are kept
as constants in tests/slot_model.py and re-checked with se_hash where they are used."""
import numpy as np
import pytest

import slot_model as sm
from slot_model import Strings, Tuples
from theia_amd import TadError, _capi as capi
from job_helpers import SKIP, STAGE, column, device_column, exported, host

pytestmark = pytest.mark.gpu

KEY_MISS = int(SKIP)
LONG = bytes(0x61 + (i * 7) % 26 for i in range(STAGE + 1000))       # one string longer than the stage: its 256-row block reads from global memory


# ---- the reference: a plain dict, ids in order of first appearance ----
class Ref:
    def __init__(self, miss):
        self.ids, self.miss = {}, miss      # miss: what the dictionary answers for a key it does not hold

    def encode(self, keys):
        """keys in VIRTUAL order ([side a ++ side b] of one call) -> their ids"""
        return [self.ids.setdefault(k, len(self.ids)) for k in keys]

    def lookup(self, keys):
        return [self.ids.get(k, self.miss) for k in keys]

    def values(self):
        return sorted(self.ids, key=self.ids.get)


def first_appearance(rows):
    """rows: keys (hashable) or None for a row that is not kept -> (ids with None where not kept, first rows)"""
    ids, first, out = {}, [], []
    for r, k in enumerate(rows):
        if k is None:
            out.append(None)
            continue
        if k not in ids:
            ids[k] = len(ids)
            first.append(r)
        out.append(ids[k])
    return out, first


# ---- the two dictionaries behind one face: keys are (side, tuple) / bytes as tests/slot_model.py makes them ----
def tuple_columns(keys):
    return [np.array([k[1][c] for k in keys], dtype=np.int64) for c in range(len(keys[0][1]))]


class KeyDictFace:
    miss = KEY_MISS

    def __init__(self, engine, n_cols, expected):
        self.d, self.n_cols = engine.key_dict(n_cols, expected), n_cols

    def _run(self, call, keys):
        """one call; every key a row, on its own side (the rows of the other side are masked out).  Virtual order = side a's rows, then b's."""
        cols, side = tuple_columns(keys), np.array([k[0] for k in keys])
        if not side.any():
            return host(call(cols)[0]).tolist()
        got = call(cols, side == 0, cols, side == 1)
        return np.where(side == 0, host(got[0]), host(got[1])).tolist()

    def virtual(self, keys):
        return [k for k in keys if k[0] == 0] + [k for k in keys if k[0] == 1]

    def encode(self, keys):
        return self._run(self.d.encode, keys)

    def lookup(self, keys):
        return self._run(self.d.lookup, keys)

    def export(self):
        cols, side = self.d.export()
        return [(int(s), tuple(int(c[i]) for c in cols)) for i, s in enumerate(side)]

    def load(self, keys):
        self.d.load(tuple_columns(keys), np.array([k[0] for k in keys], dtype=np.uint8))

    def compact(self, keep):
        keep = np.asarray(keep, bool)
        remap = np.full(keep.size, SKIP, dtype=np.uint64)
        remap[keep] = np.arange(int(keep.sum()), dtype=np.uint64)
        return self.d.compact(remap)

    def count(self):
        return self.d.num_keys()

    def table_bytes(self, slots, cap, keys=()):
        """nbytes() of a dictionary of `slots` slots and room for `cap` records"""
        return slots * 8 + cap * ((self.n_cols + 2) & ~1) * 8


class StringDictFace:
    miss = -1
    ARENA = 1 << 16                                   # room for every case here: the arena never grows, only table and records can

    def __init__(self, engine, _, expected):
        self.d = engine.string_dict(expected, self.ARENA)

    def virtual(self, keys):
        return list(keys)

    def encode(self, keys):
        return self.d.encode(column(list(keys)))[0].tolist()

    def lookup(self, keys):
        return self.d.lookup(column(list(keys))).tolist()

    def export(self):
        return exported(self.d)

    def load(self, keys):
        self.d.load(list(keys))

    def compact(self, keep):
        self.d.compact(np.asarray(keep, np.uint8))
        return self.d.num_values()

    def count(self):
        return self.d.num_values()

    def table_bytes(self, slots, cap, keys=None):
        """nbytes(): the arena is what create made it, or — keys given — what a compaction to these survivors makes it (twice their padded bytes)"""
        arena = self.ARENA if keys is None else 2 * sum((len(k) + 15) & ~15 for k in keys)
        return slots * 8 + cap * 16 + (arena or 16)


def open_dict(engine, fam, expected):
    return (KeyDictFace if isinstance(fam, Tuples) else StringDictFace)(engine, getattr(fam, "n_cols", 0), expected)


def hashes(keys):
    return [sm.hash_of(k) for k in keys]


def assert_holds(face, ref):
    """the export is the reference list and every value looks up to its id: a record's tuple / hash half and its slot still belong together"""
    vals = ref.values()
    assert face.count() == len(vals) and face.export() == vals
    assert face.lookup(vals) == list(range(len(vals)))


TUPLE_FAMILIES = [Tuples(1), Tuples(3), Tuples(8)]
STRING_FAMILIES = [Strings(8), Strings(24, 2), Strings(9), Strings(17, 1)]
ID = repr


# ---- the pins ----
def feed_one_by_one(face, keys, size0):
    """-> the calls after which nbytes() was no longer size0, and the size at the end"""
    grew = []
    for i, k in enumerate(keys):
        assert face.encode([k]) == [i]
        if face.d.nbytes() != size0:
            grew.append(i)
    return grew, face.d.nbytes()


@pytest.mark.parametrize("side", (0, 1), ids=("side_a", "side_b"))
@pytest.mark.parametrize("n_cols", (1, 2, 3, 7, 8))
def test_pin_tb_hash_a_modelled_cluster_doubles_a_256_slot_key_dictionary_at_the_modelled_call(engine, n_cols, side):
    fam = Tuples(n_cols, side)
    crowd = sm.with_home(fam, 256, 250, 4, 48)                       # homes 250 .. 253: the run crosses the table's end on its way
    far = sm.passed(256, hashes(crowd))
    at = next(i for i, p in enumerate(far) if p > sm.MAX_PROBE)      # the first claim that passes more than 32 slots
    assert all(p <= sm.MAX_PROBE for p in far[:at]) and at + 1 <= 64 and {255, 0} <= sm.occupied(256, hashes(crowd[:at + 1]))
    calm = sm.spread(fam, 256, at + 1)
    assert max(sm.passed(256, hashes(calm))) <= sm.MAX_PROBE
    face = open_dict(engine, fam, 128)
    size0 = face.d.nbytes()
    assert size0 == face.table_bytes(256, 128)
    grew, size1 = feed_one_by_one(face, crowd[:at + 1], size0)
    assert grew == [at] and size1 == size0 + 256 * 8                 # KD_FLAG_CLUSTER: 512 slots, after that call and no other
    assert face.lookup(crowd[:at + 1]) == list(range(at + 1)) and face.export() == list(crowd[:at + 1])
    control = open_dict(engine, fam, 128)
    grew, size1 = feed_one_by_one(control, calm, size0)
    assert grew == [] and size1 == size0
    assert control.lookup(calm) == list(range(at + 1))


PIN_LENGTHS = (7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)


def pin_family(length):
    return Strings(length, max(length // 8 - 1, 0))


@pytest.mark.parametrize("first", (250, 77), ids=("across_the_end", "inside"))
def test_pin_se_hash_a_modelled_cluster_of_every_length_doubles_a_256_slot_string_dictionary_at_the_modelled_call(engine, first):
    per = {n: sm.with_home(pin_family(n), 256, first, 4, 4) for n in PIN_LENGTHS}
    crowd = [b"", b"z", b"ab"] + [per[n][r] for r in range(4) for n in PIN_LENGTHS]      # "" and two short ones land where they land: the model counts them
    far = sm.passed(256, hashes(crowd))
    at = next(i for i, p in enumerate(far) if p > sm.MAX_PROBE)
    fed = crowd[:at + 1]
    assert all(p <= sm.MAX_PROBE for p in far[:at]) and at + 1 <= 64
    assert any(len(k) % 8 for k in fed[3:]) and any(len(k) > 16 for k in fed[3:]) and {len(k) for k in fed} >= set(PIN_LENGTHS) | {0}
    calm = [b"", b"z", b"ab"] + [pin_family(n).key(1000 + r) for r in range(4) for n in PIN_LENGTHS][:at + 1 - 3]
    assert max(sm.passed(256, hashes(calm))) <= sm.MAX_PROBE and len(calm) == len(fed)
    face = StringDictFace(engine, 0, 128)
    size0 = face.d.nbytes()
    assert size0 == face.table_bytes(256, 128) and sum((len(k) + 15) & ~15 for k in fed) < face.ARENA      # only the table can grow
    grew, size1 = feed_one_by_one(face, fed, size0)
    assert grew == [at] and size1 == size0 + 256 * 8                 # SD_FLAG_CLUSTER
    assert face.lookup(fed) == list(range(at + 1)) and face.export() == fed
    control = StringDictFace(engine, 0, 128)
    grew, size1 = feed_one_by_one(control, calm, size0)
    assert grew == [] and size1 == size0
    assert control.lookup(calm) == list(range(len(calm)))


# ---- 1. one fingerprint, two keys, met on the probe sequence (64 slots) ----
def met_on_the_probe(engine, fam, x, y):
    """x is held; between y's home and x's slot every slot is taken (fillers, each ON its home), so y's probe walks to x's slot, finds its own
    fingerprint there and has to compare."""
    hx, hy = sm.hash_of(x), sm.hash_of(y)
    assert x != y and sm.fingerprint(hx) == sm.fingerprint(hy)
    gap = (sm.home(hx, 64) - sm.home(hy, 64)) % 64
    assert gap + 2 <= 32                                            # with x and y at most 32 keys: the table stays at 64 slots
    fill_fam = Tuples(fam.n_cols, fam.side, fam.vary, start=10 ** 8) if isinstance(fam, Tuples) else Strings(fam.length, fam.chunk, start=1 << 40)
    fillers = [k for k in sm.cover(fill_fam, 64, sm.home(hy, 64), gap)]
    assert x not in fillers and y not in fillers
    held = [x] + fillers
    slots = sm.place(64, hashes(held))
    assert slots == [(sm.home(hy, 64) + gap + 0) % 64] + [(sm.home(hy, 64) + k) % 64 for k in range(gap)]      # x on its home, the fillers on theirs
    walk = sm.passes(64, set(slots), hy)
    assert walk[-1] == slots[0] and len(walk) == gap + 1            # y's probe ends ON x's slot, the next one is empty
    n = len(held)
    face = open_dict(engine, fam, 1)
    ref = Ref(face.miss)
    size0 = face.d.nbytes()
    for k in held:
        assert face.encode([k]) == ref.encode([k])
    assert face.lookup([y]) == [face.miss] == ref.lookup([y])       # the fingerprint alone is not a hit
    assert face.lookup([y, x, y]) == [face.miss, 0, face.miss]
    ref.encode(face.virtual([y, x, y]))
    assert face.encode([y, x, y]) == [n, 0, n] == ref.lookup([y, x, y])
    assert face.export() == held + [y] and face.d.nbytes() == size0
    assert_holds(face, ref)
    # the other way round: y held, x looked up
    other = open_dict(engine, fam, 1)
    assert other.encode([y]) == [0] and other.lookup([x, y]) == [other.miss, 0]
    assert other.encode([x, y, x]) == [1, 0, 1] and other.export() == [y, x]


@pytest.mark.parametrize("homes", ("equal", "within", "straddle"))
@pytest.mark.parametrize("fam", TUPLE_FAMILIES + [Tuples(8, vary=0)] + STRING_FAMILIES[:2], ids=ID)
def test_one_fingerprint_met_on_the_probe_sequence_is_two_keys(engine, fam, homes):
    """n_cols = 8 differs in the last column alone and (vary=0) in the first alone; 8-byte strings: the bytes decide; 24-byte strings: the
    bytes of the second 16-byte word decide.  "straddle": y's home is among the last 8 slots, x's among the first 8 — the probe wraps."""
    x, y = sm.fingerprint_pairs(fam, slots=64, homes=homes)[0]
    if homes == "straddle":
        assert sm.home(sm.hash_of(y), 64) >= 56 and sm.home(sm.hash_of(x), 64) < 8
    met_on_the_probe(engine, fam, x, y)


@pytest.mark.parametrize("fam,other", [(Tuples(n), Tuples(n, side=1)) for n in (1, 3, 8)] + [(Strings(8), Strings(9))], ids=ID)
def test_one_fingerprint_across_the_sides_and_across_the_lengths(engine, fam, other):
    """x on side a and y on side b (the side word of the record decides); 8 bytes against 9 (the length check decides)"""
    x, y = sm.fingerprint_pairs(fam, other, count=2_000_000, slots=64, homes="equal")[0]
    assert (x[0], y[0]) == (0, 1) if isinstance(fam, Tuples) else (len(x), len(y)) == (8, 9)
    met_on_the_probe(engine, fam, x, y)


@pytest.mark.parametrize("which", (0, 1, 2), ids=("7_and_9_bytes_one_home", "8_and_9_bytes", "9_and_14_bytes"))
def test_a_string_and_its_zero_extension_with_one_fingerprint_are_told_apart_by_the_length(engine, which):
    """x and y = the same content with zero bytes appended: in the arena, whose strings are zero-padded to 16 bytes, their bytes are THE SAME,
    so after the fingerprint only k_sd_probe's length check stands between them"""
    x, y = sm.zero_extension_pairs()[which]
    assert x.rstrip(b"\0") == y.rstrip(b"\0") and len(x) != len(y) and max(len(x), len(y)) <= 16
    met_on_the_probe(engine, Strings(8), x, y)


def rows_off_the_16_byte_grid(col, rows, which):
    """the device address of every row of `rows` that holds one of `which` is no multiple of 16: whichever of them becomes a slot's
    representative, se_same_as reads it with skip != 0"""
    at = col[1].ptr + col[0].to_host().astype(np.int64)[:-1]
    mine = [int(a) for a, r in zip(at, rows) if r in which]
    return len(mine) == sum(r in which for r in rows) > 0 and all(a % 16 for a in mine)


def test_one_fingerprint_in_a_device_column_at_an_odd_byte_offset(engine):
    """both strings NEW in one batch: the miss rows are de-duplicated by k_se_insert in a scratch table of 1024 slots (6 rows: the full-size
    table), which compares with the representative row IN THE COLUMN.  The pair shares its home in 1024 slots, so whichever of the two
    claims first, the other walks onto its slot and compares; every row of the pair lies off the 16-byte grid, so that compare of two
    DIFFERENT strings runs se_same_as with skip != 0."""
    x, y = sm.fingerprint_pairs(Strings(8), count=8_000_000, slots=1024, homes="equal")[0]
    hx, hy = sm.hash_of(x), sm.hash_of(y)
    assert sm.fingerprint(hx) == sm.fingerprint(hy) and x != y and sm.home(hx, 1024) == sm.home(hy, 1024) and sm.home(hx, 64) == sm.home(hy, 64)
    rows = [b"pad", y, x, y, x, b"tail"]
    assert len(rows) <= 512 and sm.home(hx, 1024) not in (sm.home(sm.hash_of(b"pad"), 1024), sm.home(sm.hash_of(b"tail"), 1024))
    for shift in (3, 9):
        d = engine.string_dict(1, 1)
        col = device_column(engine, rows, 32, shift)
        assert rows_off_the_16_byte_grid(col, rows, (x, y))
        codes, first, before = d.encode(col, out="host")
        assert codes.tolist() == [0, 1, 2, 1, 2, 3] and first.tolist() == [0, 1, 2, 5] and before == 0
        assert d.lookup(device_column(engine, [x, y], 64, shift + 1)).tolist() == [2, 1]
        assert exported(d) == [b"pad", y, x, b"tail"]
        d.close()


# ---- 2. a cluster across the table's end ----
@pytest.mark.parametrize("fam", TUPLE_FAMILIES + [Tuples(3, side=1)] + STRING_FAMILIES, ids=ID)
def test_a_cluster_that_wraps_from_the_last_slot_to_slot_0(engine, fam):
    cluster = list(sm.with_home(fam, 64, 59, 5, 10))                # ten keys whose homes are the last five slots
    stranger, newcomer = sm.with_home(fam, 64, 59, 5, 2, skip=10)
    slots = sm.place(64, hashes(cluster))
    occ = set(slots)
    assert occ == set(range(59, 64)) | set(range(5)) and len(cluster) <= 32
    behind = [k for k, s in zip(cluster, slots) if s < 59]          # held behind the wrap
    assert len(behind) == 5
    for k in (stranger, newcomer):
        walk = sm.passes(64, occ, sm.hash_of(k))
        assert 63 in walk and walk[walk.index(63) + 1] == 0 and walk[-1] == 4
    face = open_dict(engine, fam, 1)
    ref = Ref(face.miss)
    size0 = face.d.nbytes()
    for k in cluster:
        assert face.encode([k]) == ref.encode([k])
    assert face.lookup(behind) == ref.lookup(behind) and face.lookup(cluster[::-1]) == list(range(10))[::-1]      # known keys, found after the wrap
    assert face.lookup([stranger, cluster[7], newcomer]) == [face.miss, 7, face.miss]                              # an unknown key whose probe wraps: a miss
    assert sm.place(64, hashes(cluster + [newcomer]))[-1] == 5
    assert face.encode([newcomer, cluster[9]]) == [10, 9] == ref.encode([newcomer, cluster[9]])                    # appended across the wrap
    assert face.lookup([stranger]) == [face.miss] and face.d.nbytes() == size0
    assert_holds(face, ref)


# ---- 3. the load edge, and growth with a wrapping cluster inside ----
@pytest.mark.parametrize("fam", TUPLE_FAMILIES + STRING_FAMILIES[:3], ids=ID)
def test_the_33rd_key_grows_a_64_slot_table_and_the_wrapping_cluster_is_found_in_128_slots(engine, fam):
    cluster = list(sm.with_home(fam, 64, 59, 5, 10))
    keys = cluster + [k for k in (fam.key(i) for i in range(40)) if k not in cluster][:23]
    assert len(keys) == 33 and len(set(keys)) == 33
    assert {63, 0} <= sm.occupied(64, hashes(keys[:32]))
    face = open_dict(engine, fam, 1)
    ref = Ref(face.miss)
    size0 = face.d.nbytes()
    assert size0 == face.table_bytes(64, 32)
    assert face.encode(keys[:32]) == ref.encode(keys[:32]) == list(range(32))
    assert face.d.nbytes() == size0                                 # exactly 32 keys in 64 slots: load 1/2, nothing grows
    assert_holds(face, ref)
    assert face.encode(keys[32:]) == [32] == ref.encode(keys[32:])
    assert face.d.nbytes() == face.table_bytes(128, 64)             # the 33rd: 128 slots (and room for 64 records) before the append
    assert face.lookup(keys) == list(range(33))
    assert face.encode(keys[::-1]) == list(range(33))[::-1] and face.count() == 33      # re-encoding creates nothing
    assert_holds(face, ref)


# ---- 4. a rehash into a SMALLER table clusters survivors that were apart ----
@pytest.mark.parametrize("fam", TUPLE_FAMILIES + STRING_FAMILIES[:3], ids=ID)
def test_compaction_rehashes_the_survivors_into_a_64_slot_table_where_they_wrap(engine, fam):
    survivors = list(sm.with_home(fam, 64, 59, 5, 10))
    retired = [k for k in (fam.key(i) for i in range(60)) if k not in survivors][:30]
    order = [k for pair in zip(retired[:10], survivors) for k in pair] + retired[10:]       # old ids: the survivors are 1, 3, .. 19
    m = len(survivors)
    assert max(64, 1 << (4 * m - 1).bit_length()) == 64             # pow2_at_least(4 m), below the 256 slots it has
    assert sm.occupied(64, hashes(survivors)) == set(range(59, 64)) | set(range(5))
    assert len({sm.home(h, 256) // 64 for h in hashes(survivors)}) > 1      # apart before: homes in several quarters of the 256 slots
    face = open_dict(engine, fam, 100)
    ref = Ref(face.miss)
    assert face.d.nbytes() == face.table_bytes(256, 100)
    assert face.encode(order) == ref.encode(order)
    keep = [k in survivors for k in order]
    assert face.compact(keep) == m
    assert face.d.nbytes() == face.table_bytes(64, 32, survivors)   # 64 slots: the table the model was asked about
    after = Ref(face.miss)
    after.encode(survivors)
    assert face.lookup(order) == after.lookup(order)                # a survivor: its remapped id; a retired key: a miss
    assert_holds(face, after)
    newcomer = sm.with_home(fam, 64, 59, 5, 1, skip=10)[0]
    assert newcomer not in order
    assert face.encode([retired[0], newcomer, survivors[3]]) == [m, m + 1, 3] == after.encode([retired[0], newcomer, survivors[3]])
    assert_holds(face, after)


# ---- 5. import ----
@pytest.mark.parametrize("fam", TUPLE_FAMILIES + STRING_FAMILIES[:3], ids=ID)
def test_import_takes_a_same_fingerprint_pair_and_refuses_a_duplicate_behind_a_wrapping_run(engine, fam):
    if fam == Strings(9):                                           # 8 bytes against 9: the lengths decide
        x, y = sm.fingerprint_pairs(Strings(8), fam, count=2_000_000, slots=64, homes="equal")[0]
    else:
        x, y = sm.fingerprint_pairs(fam, slots=64, homes="equal")[0]
    assert sm.fingerprint(sm.hash_of(x)) == sm.fingerprint(sm.hash_of(y)) and sm.home(sm.hash_of(x), 64) == sm.home(sm.hash_of(y), 64)      # they meet, whoever claims first
    run = [k for k in sm.with_home(fam, 64, 59, 5, 12) if k not in (x, y)][:10]
    good = [x] + run + [y]
    face = open_dict(engine, fam, 1)
    ref = Ref(face.miss)
    face.load(good)
    ref.encode(good)
    assert_holds(face, ref)                                         # the neighbour with the same fingerprint is not a duplicate
    # a true duplicate: its copies are the first and the last record, or it comes behind the run that fills the slots from its home across
    # the table's end — whichever copy is hashed second has to find the first one where the run pushed it
    dup = run[0]
    assert {63, 0} <= sm.occupied(64, hashes(run)) and sm.place(64, hashes(run[1:] + [dup]))[-1] < 59
    for bad in ([dup] + run[1:] + [dup], run[1:] + [dup, x, dup], [dup, dup] + run[1:]):
        e = open_dict(engine, fam, 1)
        with pytest.raises(TadError) as ei:
            e.load(bad)
        assert ei.value.code == capi.TAD_ERR_INVALID_ARGUMENT and e.count() == 0 and e.export() == []
        e.load(good)                                                # unchanged and usable
        assert e.export() == good and e.lookup([y, dup, x]) == [len(good) - 1, 1, 0]
    if isinstance(fam, Tuples):
        # recode: the identity changes nothing (and stops after its check); a remap that moves ONE bystander's value fills a fresh table
        # through the duplicate check, which must again leave the pair alone
        col = fam.n_cols - 1
        top = max(k[1][col] for k in good) + 2
        ident = np.arange(top, dtype=np.int64)
        assert face.d.recode({col: ident}) == len(good)
        assert_holds(face, ref)
        moved = ident.copy()
        moved[run[4][1][col]] = top - 1
        assert top - 1 not in [k[1][col] for k in good]
        assert face.d.recode({col: moved}) == len(good)
        new4 = (run[4][0], run[4][1][:col] + (top - 1,))
        want = Ref(face.miss)
        want.encode([x] + run[:4] + [new4] + run[5:] + [y])
        assert_holds(face, want)
        assert face.lookup([run[4]]) == [face.miss]


# ---- tad_factorize ----
FZ = Tuples(2)


def factorize_check(engine, rows_a, keep_a=None, rows_b=None, keep_b=None):
    """rows: lists of tuples.  ids and first rows against the dict over the kept virtual rows [side a ++ side b]"""
    n = len(rows_a)
    virtual = [(0, t) if keep_a is None or keep_a[i] else None for i, t in enumerate(rows_a)]
    if rows_b is not None:
        virtual += [(1, t) if keep_b is None or keep_b[i] else None for i, t in enumerate(rows_b)]
    ids, first = first_appearance(virtual)
    want = np.array([KEY_MISS if i is None else i for i in ids], dtype=np.uint64)
    cols = lambda rows: [np.array([t[c] for t in rows], dtype=np.int64) for c in range(len(rows[0]))]
    k1, k2, fr = engine.factorize(cols(rows_a), None if keep_a is None else np.asarray(keep_a, bool), None if rows_b is None else cols(rows_b),
                                  None if keep_b is None else np.asarray(keep_b, bool))
    assert np.array_equal(k1, want[:n]) and np.array_equal(fr, np.array(first, dtype=np.uint64))
    assert (k2 is None) == (rows_b is None) and (rows_b is None or np.array_equal(k2, want[n:]))
    return ids, first


def repeated_rows(keys):
    """300 keys, every key 1 to 4 times, the copies of one key in different wavefronts (64 rows) and a key's FIRST row often on a higher lane
    than a later copy.  Wavefronts 0 - 3: keys 0 .. 255 once; 4: the second copies of every fourth of them; 5: keys 256 .. 299 and third
    copies; 6: second copies of the late keys, more third copies and the fourth ones."""
    n = len(keys)
    assert n == 300
    pick = lambda cond: [i for i in range(n) if cond(i)]
    rows = (list(range(256)) + pick(lambda i: i % 4 == 0 and i < 256) + list(range(256, n)) + pick(lambda i: i % 8 == 0 and i < 160) +
            pick(lambda i: i % 4 == 0 and i >= 256) + pick(lambda i: i % 8 == 0 and 160 <= i < 256) + pick(lambda i: i % 16 == 0 and i < 160))
    where = {}
    for r, i in enumerate(rows):
        where.setdefault(i, []).append(r)
    many = [w for w in where.values() if len(w) > 1]
    assert len(where) == n and sorted({len(w) for w in where.values()}) == [1, 2, 3, 4] and len(rows) <= 512
    assert all(len({r // 64 for r in w}) == len(w) for w in many)
    assert sum(w[0] % 64 > min(r % 64 for r in w[1:]) for w in many) >= len(many) // 2
    return [keys[i] for i in rows]


def fz_cluster():
    keys = sm.with_home(FZ, 1024, 1012, 24, 300)                    # 300 keys with homes in the last 12 and the first 12 slots
    occ = sm.occupied(1024, hashes(keys))
    assert {1023, 0} <= occ and len(occ) == 300 and max(sm.passed(1024, hashes(keys))) > 200
    return keys


def test_factorize_full_size_table_takes_a_wrapping_cluster_of_300_with_unlimited_probing(engine):
    """at most 512 virtual rows: a 1024-slot table, which IS the full-size one — no probe limit, the pass must finish in one attempt's table"""
    keys = fz_cluster()
    once = [k[1] for k in keys]
    assert len(once) <= 512
    factorize_check(engine, once)
    again = [k[1] for k in repeated_rows(keys)]                     # the atomic min on slots deep inside the cluster
    assert 300 < len(again) <= 512
    factorize_check(engine, again)
    half = len(again) // 2                                          # two sides: the same tuples are other keys on side b
    factorize_check(engine, again[:half], None, again[half:2 * half][::-1], None)


@pytest.mark.parametrize("sides", (1, 2))
def test_factorize_keeps_a_same_fingerprint_pair_apart_inside_the_cluster(engine, sides):
    x, y = sm.fingerprint_pairs(FZ, count=8_000_000, slots=1024, homes="equal")[0]
    hx = sm.hash_of(x)
    assert sm.fingerprint(hx) == sm.fingerprint(sm.hash_of(y)) and sm.home(hx, 1024) == sm.home(sm.hash_of(y), 1024)     # one home: they meet in any claim order
    crowd = [k for k in sm.with_home(FZ, 1024, (sm.home(hx, 1024) - 6) % 1024, 12, 82) if k not in (x, y)][:80]
    assert sm.home(hx, 1024) in sm.occupied(1024, hashes(crowd))
    rows = []
    for i, k in enumerate(crowd):                                   # x and y twenty times each, y first, among the crowd: 120 rows, two wavefronts
        rows.append(k[1])
        if i % 4 == 1:
            rows.append((y if i % 8 == 1 else x)[1])
        if i % 4 == 3:
            rows.append((x if i % 8 == 3 else y)[1])
    assert rows.count(x[1]) == 20 and rows.count(y[1]) == 20 and len(rows) == 120
    assert 2 * len(rows) <= 512                                     # one side or two: the 1024-slot table
    if sides == 1:
        factorize_check(engine, rows)
    else:
        factorize_check(engine, rows, None, rows[::-1], None)


def test_factorize_with_a_keep_mask_gives_dropped_rows_no_slot(engine):
    keys = fz_cluster()
    rows = repeated_rows(keys)
    dropped = set(keys[1::2])
    keep = [k not in dropped for k in rows]
    kept = [k for k in keys if k not in dropped]
    occ = sm.occupied(1024, hashes(kept))
    assert len(occ) == 150 and {1023, 0} <= occ
    ids, first = factorize_check(engine, [k[1] for k in rows], keep)
    assert [rows[r] for r in first] == [k for k in dict.fromkeys(rows) if k not in dropped]      # the kept keys, in their order


def probe_limit_rows(fam, n, crowd_size, width=32):
    """n rows, most of them repeats of five spread keys; among them `crowd_size` distinct keys whose homes lie in `width` slots of the
    2^20-slot table the first attempt uses.  -> (rows, crowd)"""
    big = 1 << 20
    crowd = sm.with_home(fam, big, big - 10, width, crowd_size)
    base = [fam.key(i) for i in range(5)]
    assert not set(base) & set(crowd) and not any(sm.in_window(sm.home(sm.hash_of(k), big), big, big - 200, 400) for k in base)
    rows = [base[i % 5] for i in range(n)]
    for i, k in enumerate(crowd):                                   # each crowd key three times, spread over the rows
        for r in (4099 + 7919 * i, 3 + 7919 * i + n // 3, n - 1 - 13 * i):
            rows[r % n] = k
    assert set(crowd) <= set(rows)
    return rows, crowd


def assert_probe_limit_is_reached(keys, width):
    """Whatever the claim order: the keys' homes lie in `width` slots, the run they fill is len(keys) slots long, so the key that claims the
    run's last slot passed at least len(keys) - width slots: more than the limit of 32.  And nothing else can ask for a larger table."""
    big = 1 << 20
    assert all(sm.in_window(sm.home(h, big), big, big - 10, width) for h in hashes(keys))
    assert len(set(keys)) - width > sm.MAX_PROBE and max(sm.passed(big, hashes(keys))) > sm.MAX_PROBE
    assert 2 * (len(keys) + 5) < big // 100                         # load under 1 %


@pytest.mark.parametrize("masked", (False, True), ids=("all_rows", "every_other_crowd_key_dropped"))
def test_factorize_probe_limit_at_low_load_repeats_the_pass_on_the_next_table(engine, masked):
    """More than 2^19 rows: the first table has 2^20 slots and is not the full-size one, so the probe limit of 32 holds there.  The pass is
    abandoned mid-flight (FZ_FLAG_GROW raised by the probe limit alone), k_fz_ids and k_fz_lookup return at once and the host repeats it
    with 2^21 slots.  The engine exposes no count of attempts: that the retry happens rests on the model, and the model on the pins."""
    n = 600_000
    rows, crowd = probe_limit_rows(FZ, n, 140 if masked else 70)
    assert n > 1 << 19 and max(1024, 1 << (2 * n - 1).bit_length()) > 1 << 20
    dropped = set(crowd[1::2]) if masked else set()
    assert_probe_limit_is_reached([k for k in crowd if k not in dropped], 32)
    keep = [k not in dropped for k in rows] if masked else None
    factorize_check(engine, [k[1] for k in rows], keep)


GRID_ROWS = 16384 * 256          # the insert kernels launch at most 16384 workgroups of 256: from here on a thread takes a second row


def late_claim_rows(fam):
    """More rows than the insert pass has threads: thread j takes row j and then row GRID_ROWS + j.  A key whose copies sit at rows 256 + j
    (workgroup 1, first round) and GRID_ROWS + j' (workgroup 0, second round) is claimed for its LATER row wherever workgroup 0 has finished
    two rounds before workgroup 1 starts — always where the workgroups run one after the other, sometimes on the device — and the earlier
    row then has to lower the slot with the atomic min.  (On the device the race is met the other way round too: repeated_rows puts the
    copies of a key into different wavefronts of a launch whose threads take one row each.)  The keys that do this are a cluster of 24 in
    an 8-slot window across the end of the 2^20-slot table (no claim passes more than 32: one attempt), their slots behind other keys'
    slots; the other rows repeat five spread keys.  -> (the key table, the rows as indices into it)"""
    big = 1 << 20
    crowd = sm.with_home(fam, big, big - 4, 8, 24)
    table = [fam.key(i) for i in range(5)] + list(crowd)
    assert len(set(table)) == 29 and max(sm.passed(big, hashes(table))) <= sm.MAX_PROBE and {big - 1, 0} <= sm.occupied(big, hashes(table))
    n = GRID_ROWS + 512
    idx = np.arange(n, dtype=np.int64) % 5
    for j in range(24):
        idx[256 + 3 * j] = 5 + j                                    # workgroup 1, first round: the key's FIRST row
        idx[GRID_ROWS + 3 * j + 1] = 5 + j                          # workgroup 0, second round: a later row, taken by an early thread
        idx[GRID_ROWS + 300 + j] = 5 + j                            # and one more in workgroup 1's second round
    return table, idx


def test_factorize_lowers_a_slot_claimed_for_a_later_row(engine):
    table, idx = late_claim_rows(FZ)
    ids, first = first_appearance(idx.tolist())                     # (the keys of the table are distinct: their indices stand for them)
    assert first[5:] == [256 + 3 * j for j in range(24)]
    cols = [np.array([k[1][c] for k in table], dtype=np.int64)[idx] for c in range(2)]
    k1, _, fr = engine.factorize(cols)
    assert np.array_equal(k1, np.array(ids, dtype=np.uint64)) and np.array_equal(fr, np.array(first, dtype=np.uint64))


def test_encode_strings_lowers_a_slot_claimed_for_a_later_row(engine):
    table, idx = late_claim_rows(Strings(12, 1))
    ids, first = first_appearance(idx.tolist())
    assert first[5:] == [256 + 3 * j for j in range(24)]
    data = np.frombuffer(b"".join(table), dtype=np.uint8).reshape(len(table), 12)[idx].reshape(-1)
    codes, fr = engine.encode_strings((np.arange(idx.size + 1, dtype=np.int64) * 12, data))
    assert np.array_equal(codes, np.array(ids, dtype=np.int64)) and np.array_equal(fr, np.array(first, dtype=np.uint64))


# ---- tad_encode_strings ----
def encode_strings_check(engine, rows, over_stage):
    """codes, first rows and the dictionary against the dict of first appearance.  over_stage: the long string at the head of every 256-row
    block puts every block's bytes over kSeStage — all compares read global memory; else every block is staged in LDS."""
    rows = list(rows)
    if over_stage:
        r = 0
        while r < len(rows):
            rows.insert(r, LONG)
            r += 256
    spans = [sum(len(s) for s in rows[r:r + 256]) for r in range(0, len(rows), 256)]
    assert all(s > STAGE for s in spans) if over_stage else all(s + 16 <= STAGE for s in spans)
    ids, first = first_appearance(rows)
    off, data = column(rows)
    codes, fr = engine.encode_strings((off, data))
    assert np.array_equal(codes, np.array(ids, dtype=np.int64)) and np.array_equal(fr, np.array(first, dtype=np.uint64))
    assert [rows[int(r)] for r in fr] == list(dict.fromkeys(rows))
    return rows, ids, first


def se_cluster(per_length):
    keys = [k for r in range(per_length) for n in PIN_LENGTHS for k in (sm.with_home(pin_family(n), 1024, 1012, 24, per_length)[r],)]
    occ = sm.occupied(1024, hashes(keys))
    assert {1023, 0} <= occ and len(set(keys)) == len(keys) and max(sm.passed(1024, hashes(keys))) > len(keys) - 40
    return keys


@pytest.mark.parametrize("over_stage", (False, True), ids=("staged_in_lds", "from_global_memory"))
def test_encode_strings_full_size_table_takes_a_wrapping_cluster_of_every_length(engine, over_stage):
    keys = se_cluster(25)                                           # 300 strings of 7 .. 33 bytes with homes around the table's end
    assert len(keys) == 300
    encode_strings_check(engine, keys, over_stage)
    again = repeated_rows(keys)
    assert len(again) + 2 <= 512                                    # with the two long rows: still the 1024-slot, full-size table
    encode_strings_check(engine, again, over_stage)


@pytest.mark.parametrize("over_stage", (False, True), ids=("staged_in_lds", "from_global_memory"))
def test_encode_strings_keeps_a_same_fingerprint_pair_apart_inside_the_cluster(engine, over_stage):
    x, y = sm.fingerprint_pairs(Strings(8), count=8_000_000, slots=1024, homes="equal")[0]
    hx = sm.hash_of(x)
    assert sm.fingerprint(hx) == sm.fingerprint(sm.hash_of(y)) and sm.home(hx, 1024) == sm.home(sm.hash_of(y), 1024) and x != y
    crowd = [k for n in (7, 9, 16, 17, 24, 33) for k in sm.with_home(pin_family(n), 1024, (sm.home(hx, 1024) - 6) % 1024, 12, 12)]
    assert sm.home(hx, 1024) in sm.occupied(1024, hashes(crowd))
    rows = []
    for i, k in enumerate(crowd):
        rows.append(k)
        if i % 4 == 1:
            rows.append(y if i % 8 == 1 else x)
        if i % 4 == 3:
            rows.append(x if i % 8 == 3 else y)
    assert rows.count(x) == 18 and rows.count(y) == 18 and len(rows) <= 510
    encode_strings_check(engine, rows, over_stage)
    if not over_stage:
        # and from device buffers: the strings of 8, 16 and 24 bytes behind a 3-byte one, so that every row starts 3 + shift bytes off the
        # 8-byte grid — whichever row of x or y becomes the representative, the compare of the two reads it with skip != 0
        dev_rows = [b"pad"] + [r for r in rows if len(r) % 8 == 0]
        assert dev_rows.count(x) == 18 and dev_rows.count(y) == 18 and len(dev_rows) <= 512
        ids, first = first_appearance(dev_rows)
        for shift in (2, 10):
            col = device_column(engine, dev_rows, 32, shift)
            assert rows_off_the_16_byte_grid(col, dev_rows, (x, y))
            codes, fr = engine.encode_strings((col[0], col[1]))
            assert codes.to_host().tolist() == ids and fr.to_host().tolist() == first


@pytest.mark.parametrize("over_stage", (False, True), ids=("staged_in_lds", "from_global_memory"))
def test_encode_strings_probe_limit_at_low_load_repeats_the_pass_on_the_next_table(engine, over_stage):
    """tad_factorize's case over strings: more than 2^19 rows of mostly repeated short strings, 70 distinct 12-byte strings with homes in 32
    slots of the 2^20-slot table.  SE_FLAG_GROW is raised by the probe limit alone; the retry is reached by construction (model, pins)."""
    n = 600_000
    fam = Strings(12, 1)
    rows, crowd = probe_limit_rows(fam, n, 70)
    assert_probe_limit_is_reached(list(crowd), 32)
    encode_strings_check(engine, rows, over_stage)
