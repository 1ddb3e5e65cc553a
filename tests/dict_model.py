"""A host model of the two dictionaries of the streaming path (include/tad.h: tad_keydict, tad_strdict) and seeded operation scripts
over it — a helper module, no tests in it.

include/tad.h defines every dictionary call as a function of what the dictionary holds: the values of a vocabulary in code order, the
(side, tuple) keys of a key dictionary in id order.  VocabModel and KeyDictModel keep exactly that — a Python list plus a dict — and
restate each call's rule over it in plain Python / numpy; DictSetModel is one key dictionary with the vocabularies of its string columns
(two columns may share one).  The LIKE language comes from tests/like_ref.py.  No engine call, no device, no hash on this side: where a
value sits in a table, and at which capacity, is the product's business — `_Caps` below restates only the documented size rules, for
the coverage assertions of tests/test_dict_model.py.

make_script(seed) draws twelve operations with every argument fixed and every precondition decided on the model alone.
tests/test_dict_model.py checks the model and what the seed set covers on the host; tests/test_gpu_dict_sequences.py runs the scripts
on a KeyDict and its StringDicts (tests/dict_drivers.py) and compares after every operation.

Not covered, on purpose: concurrent calls on one dictionary, workspace-limit refusals, more than 2^32 of anything (rows, keys, values,
bytes of one string), Unicode case folding (the product folds 'A'..'Z' only, and so does this model), a streaming state next to the
dictionaries (tests/test_gpu_stream_retire.py runs the three together)."""
import functools

import numpy as np

import like_ref
import slot_model as S

U64, I64, U8 = np.uint64, np.int64, np.uint8
KEY_SKIP = U64(0xFFFFFFFFFFFFFFFF)
CODE_NONE = -1
STR_EQUAL, STR_CONTAINS_NOCASE = 0, 1
MAX_PATTERN = 1024
SEEDS = tuple(range(32))
N_OPS = 12
CLASSES = ("growth", "wide", "long", "churn", "collide")
KINDS = ("encode", "lookup", "select", "decode", "restart", "compact_keys", "retire_strings", "refused")
CHECK_KINDS = ("select", "decode", "like")
SURVIVORS = ("share", "all", "none", "prefix", "last", "but_first")
REFUSALS = ("remap_swapped", "remap_duplicate", "remap_gap", "remap_wrong_length", "recode_to_none", "recode_makes_equal", "column_twice",
            "stale_keep_len", "match_stale_mask_len", "like_stale_mask_len", "import_nonempty", "import_duplicate", "offsets_decrease",
            "gather_num_keys", "decode_num_values", "mark_used_len_below")
LONG_LENGTHS = (0, 1, 15, 16, 17, 127, 128, 129, 4095, 4096, 4097, 16400)


class Refused(Exception):
    """the call must be refused (TAD_ERR_INVALID_ARGUMENT) and leave everything as it was"""


def up16(x):
    return (x + 15) & ~15


def arrow(strings):
    """a list of bytes -> (offsets int64[n + 1], data uint8[...]): Arrow's layout as export and decode write it"""
    off = np.zeros(len(strings) + 1, I64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return off, np.frombuffer(b"".join(strings), dtype=U8).copy()


def fold(b):
    return b.translate(like_ref.FOLD)


# ---- the vocabulary: tad_strdict ----
class VocabModel:
    """the values in code order"""

    def __init__(self, values=()):
        self.values = list(values)
        self.index = {v: c for c, v in enumerate(self.values)}
        assert len(self.index) == len(self.values)

    def __len__(self):
        return len(self.values)

    def encode(self, strings, max_new=None):
        """-> (codes, new_first_row, num_before): new values are numbered in order of first appearance; the list is capped, the codes never"""
        before, first = len(self.values), []
        codes = np.empty(len(strings), I64)
        for r, s in enumerate(strings):
            c = self.index.get(s)
            if c is None:
                c = self.index[s] = len(self.values)
                self.values.append(s)
                first.append(r)
            codes[r] = c
        cap = len(strings) if max_new is None else max_new
        return codes, np.array(first[:cap], U64), before

    def lookup(self, strings):
        return np.array([self.index.get(s, CODE_NONE) for s in strings], I64)

    def export(self, first=0, n=None):
        return arrow(self.values[first:] if n is None else self.values[first:first + n])

    def load(self, values):
        if self.values or len(set(values)) != len(values):
            raise Refused("import into a vocabulary that holds values, or of two equal strings")
        self.__init__(values)

    def decode(self, codes):
        codes = np.asarray(codes, I64)
        if ((codes < 0) | (codes >= len(self.values))).any():
            raise Refused("a code outside [0, num_values)")
        return arrow([self.values[c] for c in codes.tolist()])

    def padded(self):
        """arena_used: every value zero-padded to a multiple of 16 bytes"""
        return sum(up16(len(v)) for v in self.values)

    def compact(self, keep):
        """-> (remap, stats): value c survives iff keep[c] != 0, the survivors renumbered densely in order"""
        keep = np.asarray(keep)
        if keep.size != len(self.values):
            raise Refused("keep_len != num_values")
        stats = {"values_before": len(self.values), "arena_used_before": self.padded()}
        alive = keep != 0
        remap = np.where(alive, np.cumsum(alive) - 1, CODE_NONE).astype(I64)
        self.__init__([v for v, a in zip(self.values, alive.tolist()) if a])
        stats.update(values_after=len(self.values), arena_used_after=self.padded())
        return remap, stats

    def match(self, op, pattern):
        if len(pattern) > MAX_PATTERN:
            raise Refused("pattern over 1024 bytes")
        if op == STR_EQUAL:
            m = [1 if v == pattern else 0 for v in self.values]
        else:
            p = fold(pattern)
            m = [1 if p in fold(v) else 0 for v in self.values]
        return np.array(m, U8), int(sum(m))

    def like(self, pattern, nocase):
        if len(pattern) > MAX_PATTERN:
            raise Refused("pattern over 1024 bytes")
        m = like_ref.like_mask(pattern, self.values, nocase)
        return np.array(m, U8), int(sum(m))


# ---- the key dictionary: tad_keydict ----
class KeyDictModel:
    """the keys (side, tuple) in id order"""

    def __init__(self, n_cols, keys=()):
        self.n_cols = n_cols
        self.keys = list(keys)
        self.index = {k: i for i, k in enumerate(self.keys)}
        assert len(self.index) == len(self.keys)

    def __len__(self):
        return len(self.keys)

    @staticmethod
    def _virtual(a, keep_a, b, keep_b):
        """the batch's virtual rows [a ++ b] -> [(side, tuple) or None where the mask is 0]"""
        out = []
        for side, (rows, keep) in enumerate(((a, keep_a), (b, keep_b))):
            if rows is None:
                continue
            kept = np.ones(len(rows), bool) if keep is None else np.asarray(keep) != 0
            out += [(side, tuple(r)) if k else None for r, k in zip(np.asarray(rows, I64).tolist(), kept.tolist())]
        return out

    def encode(self, a, keep_a=None, b=None, keep_b=None, max_new=None):
        """a, b: int64 [n, n_cols] -> (key_id, key_id2 or None, new_first_row, num_keys_before)"""
        before, first = len(self.keys), []
        rows = self._virtual(a, keep_a, b, keep_b)
        ids = np.full(len(rows), KEY_SKIP, U64)
        for v, key in enumerate(rows):
            if key is None:
                continue
            i = self.index.get(key)
            if i is None:
                i = self.index[key] = len(self.keys)
                self.keys.append(key)
                first.append(v)
            ids[v] = i
        cap = len(rows) if max_new is None else max_new
        n = len(a)
        return ids[:n], (ids[n:] if b is not None else None), np.array(first[:cap], U64), before

    def lookup(self, a, keep_a=None, b=None, keep_b=None):
        rows = self._virtual(a, keep_a, b, keep_b)
        ids = np.array([KEY_SKIP if key is None else self.index.get(key, KEY_SKIP) for key in rows], U64)
        n = len(a)
        return ids[:n], (ids[n:] if b is not None else None)

    def export(self, first=0, n=None):
        keys = self.keys[first:] if n is None else self.keys[first:first + n]
        cols = [np.array([t[c] for _, t in keys], I64) for c in range(self.n_cols)]
        return cols, np.array([s for s, _ in keys], U8)

    def load(self, cols, side=None):
        n = len(cols[0])
        side = np.zeros(n, U8) if side is None else np.asarray(side)
        keys = [(int(side[i]), tuple(int(c[i]) for c in cols)) for i in range(n)]
        if self.keys or len(set(keys)) != len(keys) or (side > 1).any():
            raise Refused("import into a dictionary that holds keys, of two equal tuples, or of a side > 1")
        self.__init__(self.n_cols, keys)

    def gather(self, ids, cols=None):
        ids = np.asarray(ids, U64)
        if (ids >= U64(len(self.keys))).any():
            raise Refused("an id that is not below num_keys")
        want = range(self.n_cols) if cols is None else cols
        picked = [self.keys[i] for i in ids.tolist()]
        return [np.array([t[c] for _, t in picked], I64) for c in want], np.array([s for s, _ in picked], U8)

    def select(self, terms, side=None):
        """terms: [(col, mask)] -> (keep, n_selected)"""
        if len(terms) > 8 or any(not 0 <= c < self.n_cols for c, _ in terms):
            raise Refused("terms")
        keep = np.zeros(len(self.keys), U8)
        for k, (s, t) in enumerate(self.keys):
            ok = side is None or s == side
            for c, mask in terms:
                if not 0 <= t[c] < len(mask):
                    raise Refused("a key's value lies outside the mask of its term")
                ok = ok and mask[t[c]] != 0
            keep[k] = ok
        return keep, int(keep.sum())

    def mark(self, col, n_values, into=None):
        """tad_keydict_mark_codes -> (used, n_used)"""
        if not 0 <= col < self.n_cols:
            raise Refused("col")
        used = np.zeros(n_values, U8) if into is None else np.array(into, U8)
        assert used.size == n_values
        for _, t in self.keys:
            if not 0 <= t[col] < n_values:
                raise Refused("a key's value lies outside [0, used_len)")
            used[t[col]] = 1
        return used, int(np.count_nonzero(used))

    def recode(self, remaps):
        """remaps: [(col, remap)]"""
        cols = [c for c, _ in remaps]
        if len(set(cols)) != len(cols) or len(cols) > 8 or any(not 0 <= c < self.n_cols for c in cols):
            raise Refused("a column named twice or out of range")
        new = []
        for s, t in self.keys:
            t = list(t)
            for c, r in remaps:
                if not 0 <= t[c] < len(r) or r[t[c]] == CODE_NONE:
                    raise Refused("a value outside its remap or mapped to TAD_CODE_NONE")
                t[c] = int(r[t[c]])
            new.append((s, tuple(t)))
        if len(set(new)) != len(new):
            raise Refused("two keys whose recoded tuples are equal")
        self.__init__(self.n_cols, new)
        return len(new)

    def compact(self, remap):
        remap = np.asarray(remap, U64)
        alive = remap != KEY_SKIP
        if remap.size != len(self.keys) or not np.array_equal(remap[alive], np.arange(int(alive.sum()), dtype=U64)):
            raise Refused("remap: a wrong length, or its entries are not 0 .. m - 1 in order")
        self.__init__(self.n_cols, [k for k, a in zip(self.keys, alive.tolist()) if a])
        return len(self.keys)


# ---- the pair ----
class DictSetModel:
    """one key dictionary of n_cols columns; str_cols = {column: vocabulary index}: those columns hold codes of that vocabulary"""

    def __init__(self, n_cols, str_cols):
        self.n_cols, self.str_cols = n_cols, dict(str_cols)
        self.vocabs = [VocabModel() for _ in range(1 + max(self.str_cols.values()))]
        self.keys = KeyDictModel(n_cols)

    def cols_of(self, v):
        return [c for c in sorted(self.str_cols) if self.str_cols[c] == v]

    def snapshot(self):
        cols, side = self.keys.export()
        return {"num_keys": len(self.keys), "key_cols": cols, "key_side": side, "num_values": [len(v) for v in self.vocabs],
                "values": [list(v.values) for v in self.vocabs]}

    def raw_key(self, key):
        """a key with its codes replaced by their strings"""
        s, t = key
        return s, tuple(self.vocabs[self.str_cols[c]].values[x] if c in self.str_cols else x for c, x in enumerate(t))

    def raw_keys(self):
        return [self.raw_key(k) for k in self.keys.keys]


def effective(strings, nulls):
    """the strings a column encodes: a null row encodes like "", even when it still owns bytes"""
    return strings if nulls is None else [b"" if z else s for s, z in zip(strings, nulls.tolist())]


def string_steps(model, op):
    """the string columns of a batch in the order they go through their vocabularies: by column, side a before side b"""
    return [(c, s) for c in sorted(model.str_cols) for s in range(op["sides"])]


def tuples_of(model, op, codes):
    """-> [side a rows, side b rows or None] as int64 [n, n_cols]: the int columns as drawn, the string columns as the codes given"""
    out = []
    for s in range(2):
        if s >= op["sides"]:
            out.append(None)
            continue
        out.append(np.stack([codes[(c, s)] if c in model.str_cols else op["ints"][s][c] for c in range(model.n_cols)], axis=1).astype(I64)
                   if op["n"] else np.zeros((0, model.n_cols), I64))
    return out


def survivors_remap(alive):
    alive = np.asarray(alive, bool)
    return np.where(alive, (np.cumsum(alive) - 1).astype(U64), KEY_SKIP).astype(U64)


def apply(model, op):
    """one operation on the model -> the outputs the call(s) must return, in the form dict_drivers.execute gives them"""
    kind = op["kind"]
    if kind in ("encode", "lookup"):
        codes, out = {}, {"str": []}
        for c, s in string_steps(model, op):
            strings, nulls = op["strs"][s][c]
            voc, eff = model.vocabs[model.str_cols[c]], effective(strings, nulls if op["forms"][(c, s)]["validity"] else None)
            if kind == "encode":
                cd, first, before = voc.encode(eff, op["str_max_new"][(c, s)])
                out["str"].append({"codes": cd, "first": first, "before": before, "after": len(voc)})
            else:
                cd = voc.lookup(eff)
                out["str"].append({"codes": cd})
            codes[(c, s)] = cd
        a, b = tuples_of(model, op, codes)
        if kind == "encode":
            out["key1"], out["key2"], out["first"], out["before"] = model.keys.encode(a, op["keep_a"], b, op["keep_b"], op["max_new"])
        else:
            out["key1"], out["key2"] = model.keys.lookup(a, op["keep_a"], b, op["keep_b"])
        out["num_keys"] = len(model.keys)
        return out
    if kind == "select":
        masks = []
        for t in op["terms"]:
            voc = model.vocabs[model.str_cols[t["col"]]]
            masks.append(voc.like(t["pattern"], t["nocase"]) if t["how"] == "like" else voc.match(t["op"], t["pattern"]))
        keep, n = model.keys.select([(t["col"], m) for t, (m, _) in zip(op["terms"], masks)], op["side"])
        return {"masks": masks, "keep": keep, "n_selected": n}
    if kind == "like":
        mask, n = model.vocabs[op["vocab"]].like(op["pattern"], op["nocase"])
        return {"mask": mask, "n_matched": n}
    if kind == "decode":
        want = list(range(model.n_cols)) if op["cols"] is None else op["cols"]
        columns, side = model.keys.gather(op["ids"], op["cols"])
        return {"columns": columns, "side": side,
                "decoded": {c: model.vocabs[model.str_cols[c]].decode(col) for c, col in zip(want, columns) if c in model.str_cols}}
    if kind == "restart":
        return {"exported": model.snapshot()}
    if kind == "compact_keys":
        return {"num_keys": model.keys.compact(op["remap"])}
    if kind == "retire_strings":
        out = {"n_used": {}, "used": {}, "remaps": {}, "stats": {}}
        for v, voc in enumerate(model.vocabs):
            used, counts = None, []
            for c in model.cols_of(v):
                used, n = model.keys.mark(c, len(voc), used)
                counts.append(n)
            keep = used.copy()
            keep[op["extras"][v]] = 1
            out["n_used"][v], out["used"][v] = counts, used
            out["remaps"][v], out["stats"][v] = voc.compact(keep)
        out["num_keys"] = model.keys.recode([(c, out["remaps"][model.str_cols[c]]) for c in sorted(model.str_cols)])
        return out
    if kind == "refused":
        try:
            refused_on_model(model, op)
        except Refused:
            return {"raises": True}
        raise AssertionError("the model accepts the refusal %s" % describe(op))
    raise ValueError(kind)


def refused_on_model(model, op):
    """the refused call on (a copy of) the model: every variant must raise Refused here, decided on the model alone"""
    v, keys = op["variant"], model.keys
    if v.startswith("remap_"):
        KeyDictModel(keys.n_cols, keys.keys).compact(op["remap"])
    elif v in ("recode_to_none", "recode_makes_equal", "column_twice"):
        KeyDictModel(keys.n_cols, keys.keys).recode(op["remaps"])
    elif v == "stale_keep_len":
        VocabModel(model.vocabs[op["vocab"]].values).compact(op["keep"])
    elif v in ("match_stale_mask_len", "like_stale_mask_len"):
        if op["mask_len"] != len(model.vocabs[op["vocab"]]):
            raise Refused("mask_len != num_values")
    elif v == "import_nonempty":
        if op["target"] == "keys":
            KeyDictModel(keys.n_cols, keys.keys).load(*op["load"])
        else:
            VocabModel(model.vocabs[op["vocab"]].values).load(op["load"])
    elif v == "import_duplicate":
        if op["target"] == "keys":
            KeyDictModel(keys.n_cols).load(*op["load"])
        else:
            VocabModel().load(op["load"])
    elif v == "offsets_decrease":
        off = op["offsets"]
        if (np.diff(off) < 0).any() or off[-1] > len(op["data"]):
            raise Refused("the offsets decrease or point beyond data_bytes")
    elif v == "gather_num_keys":
        keys.gather(op["ids"])
    elif v == "decode_num_values":
        model.vocabs[op["vocab"]].decode(op["codes"])
    elif v == "mark_used_len_below":
        keys.mark(op["col"], op["used_len"])
    else:
        raise ValueError(v)


# ---- the documented size rules, for the coverage assertions: load <= 1/2, 64 slots / 32 records / 16 arena bytes at the least ----
def pow2_at_least(x):
    s = 64
    while s < x:
        s <<= 1
    return s


class _Caps:
    """slots / records (/ arena bytes) of one dictionary as tad.h documents them; the product may hold a LARGER table (it doubles one whose
    probe sequences grow long), so a growth predicted here is a lower bound on what the product does"""

    def __init__(self, expected, expected_bytes=None):
        self.expected, self.expected_bytes = expected, expected_bytes
        self.slots = pow2_at_least(2 * expected) if expected else 1 << 20
        self.recs = max(expected, 32) if expected else 1 << 16
        self.arena = None if expected_bytes is None else (up16(expected_bytes) if expected_bytes else 4 << 20)
        self.compacted = False

    def reserve(self, total, nbytes=0):
        """room for total entries (and nbytes arena bytes) -> what grew"""
        grew = []
        if total > self.recs:
            self.recs = max(2 * self.recs, total)
            grew.append("records")
        if self.arena is not None and nbytes > self.arena:
            self.arena = up16(max(2 * self.arena, nbytes))
            grew.append("arena")
        if 2 * total > self.slots:
            self.slots = pow2_at_least(2 * total)
            grew.append("table")
        return grew

    def compact(self, before, after, nbytes=0):
        if before == after and self.arena is not None:      # a string compaction that retires nothing reallocates nothing
            return
        self.recs = min(max(2 * after, 32), self.recs)
        self.slots = min(pow2_at_least(4 * after), self.slots)
        if self.arena is not None:
            self.arena = min(2 * nbytes if nbytes else 16, self.arena)
        self.compacted = True


# ---- engineered collisions: tests/slot_model.py's hashes and searchers ----
COLLIDE_CANDIDATES = 1 << 20        # a narrower search than slot_model.PAIR_CANDIDATES (4e6): 128 same-fingerprint pairs expected, 0.2 s
ANCHOR = b"anchor"                  # the first string of a collide script: code 0, the code the engineered tuples hold in column 1


@functools.lru_cache(maxsize=None)
def collide_tuples():
    """-> (pair, cluster): values x of column 0 such that the side-0 tuples (x, 0) — column 1 holds code 0 — are a same-fingerprint pair,
    and five keys whose home slots are the last two of a 64-slot table (so of the last 66 of a 128-slot one): their claims wrap"""
    h = S.tb_hash([np.arange(COLLIDE_CANDIDATES, dtype=I64), np.int64(0)], 0)
    fp = h >> U64(32)
    order = np.argsort(fp, kind="stable")
    eq = np.flatnonzero(fp[order][1:] == fp[order][:-1])
    if eq.size == 0:
        raise LookupError("no same-fingerprint pair of tuples among %d candidates" % COLLIDE_CANDIDATES)
    pair = (int(order[eq[0]]), int(order[eq[0] + 1]))
    cluster = [int(x) for x in np.flatnonzero((h & U64(63)) >= U64(62))[:5]]
    return pair, tuple(cluster)


@functools.lru_cache(maxsize=None)
def collide_strings():
    """-> (pair, cluster) of byte strings: one fingerprint; five home slots in the last two of a 64-slot table"""
    pair = S.fingerprint_pairs(S.Strings(12), count=COLLIDE_CANDIDATES)[0]
    return tuple(pair), S.with_home(S.Strings(9), 64, 62, 2, 5)


def same_fingerprint_pair(keys):
    """do two of these keys (tuples as (side, tuple), or bytes) share a fingerprint?"""
    fps = [S.fingerprint(S.hash_of(k)) for k in keys]
    return len(set(fps)) < len(fps)


def wrapping_cluster(keys, slots=64):
    """are at least four of these keys at home in the last two slots of the table?"""
    return sum(1 for k in keys if S.home(S.hash_of(k), slots) >= slots - 2) >= 4


# ---- the scripts ----
ALPHABET = b"abzABZxyXY019_-%\\/.k"
HIGH = ["é".encode(), "日".encode(), "ß".encode(), b"\xff", b"\x80", "Z".encode(), "z".encode(), "K".encode(), b"\n"]
SPECIAL_INTS = (0, -1, 1, (1 << 63) - 1, -(1 << 63), 1 << 32, (1 << 32) - 1, -(1 << 32))


class _Gen:
    def __init__(self, seed):
        self.seed, self.cls = seed, CLASSES[seed % len(CLASSES)]
        self.rng = rng = np.random.default_rng([seed, 0xD1C7])
        cls = self.cls
        if cls == "wide":
            self.n_cols, self.str_cols, self.expected = 8, {1: 0, 4: 0, 6: 1}, (256, 256, 4096)
            pool, n_strings, self.rows = 220, (150, 60), (40, 300)
        elif cls == "long":
            self.n_cols, self.str_cols, self.expected = 2, {1: 0}, (256, 64, 1024)
            pool, n_strings, self.rows = 500, (0,), (20, 120)
        elif cls == "growth":
            self.n_cols, self.str_cols, self.expected = 3, {1: 0}, (1, 1, 1)
            pool, n_strings, self.rows = 6500, (2000,), (200, 3000)
        elif cls == "churn":
            self.n_cols, self.str_cols, self.expected = 3, {2: 0}, (1, 1, 1)
            pool, n_strings, self.rows = 7500, (4000,), (150, 900)
        else:
            self.n_cols, self.str_cols, self.expected = 2, {1: 0}, (1, 1, 1)
            pool, n_strings, self.rows = 600, (200,), (60, 300)
        self.m = DictSetModel(self.n_cols, self.str_cols)
        self.strings = [self.long_strings() if cls == "long" else self.short_strings(n) for n in n_strings]
        n_ints = max(3, int(round((pool / 4) ** (1.0 / max(1, self.n_cols - len(self.str_cols))))))
        self.ints = np.concatenate([np.array(SPECIAL_INTS, I64), rng.integers(-(1 << 62), 1 << 62, size=n_ints)])[:max(n_ints, 3)]
        self.pool = []
        for i in range(pool):                 # one tuple in eight differs from the one before it in one string column alone
            t = self.raw_tuple()
            if i % 8 == 7:
                c = sorted(self.str_cols)[int(rng.integers(len(self.str_cols)))]
                t = self.pool[-1][:c] + (t[c],) + self.pool[-1][c + 1:]
            self.pool.append(t)
        self.hi = 0                       # the rows of a batch are drawn from pool[: hi + what the batch adds]
        self.retired = []                 # raw keys that a key compaction retired
        self.refusals = self.compactions = 0
        self.kd_caps = _Caps(self.expected[0])
        self.sd_caps = [_Caps(self.expected[1], self.expected[2]) for _ in self.m.vocabs]
        self.max_keys = self.max_values = 0

    # -- the pools --
    def short_strings(self, n):
        rng, out = self.rng, {b"": None}
        while len(out) < n:
            ln = int(rng.choice([1, 2, 3, 5, 8, 13, 15, 16, 17, 24, 31, 32, 33, 40]))
            s = bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=ln))
            if rng.random() < 0.05:
                s = s[: ln // 2] + HIGH[int(rng.integers(len(HIGH)))] + s[ln // 2:]
            out[s] = None
        return list(out)

    def long_strings(self):
        """<= 300 values; every length of LONG_LENGTHS several times over: strings of one length share all but a few bytes"""
        rng, out = self.rng, {}
        for ln in LONG_LENGTHS:
            body = bytearray(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=ln))
            for j in range(0, max(ln - 8, 0), 97):                     # bytes >= 0x80 and multi-byte UTF-8, for _
                h = HIGH[int(rng.integers(len(HIGH)))]
                body[j:j + len(h)] = h
            body = bytes(body[:ln])
            out[body] = None
            for k in range(1 if ln == 0 else (3 if ln >= 4095 else 8)):
                if ln:
                    at = [0, ln - 1, ln // 2][k % 3]
                    out[body[:at] + bytes([0x61 + k]) + body[at + 1:]] = None
        while len(out) < 280:
            ln = int(rng.choice([2, 3, 7, 14, 18, 30, 33, 64, 100, 130, 200]))
            out[bytes(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), size=ln))] = None
        return list(out)

    def raw_tuple(self):
        rng = self.rng
        return tuple(self.pick_string(self.str_cols[c]) if c in self.str_cols else int(self.ints[int(rng.integers(self.ints.size))]) for c in range(self.n_cols))

    def pick_string(self, v):
        pool = self.strings[v]
        if self.cls == "long":                # the long ones are few and heavy: a row holds one with probability 1 / 6
            heavy = [s for s in pool if len(s) >= 4095]
            light = [s for s in pool if len(s) < 4095]
            src = heavy if self.rng.random() < 1 / 6 else light
            return src[int(self.rng.integers(len(src)))]
        return pool[int(self.rng.integers(len(pool)))]

    # -- batches --
    def draw_rows(self, n, fresh):
        """n raw tuples: from the pool's window, which `fresh` new entries widen first; some retired keys return"""
        rng = self.rng
        lo, self.hi = self.hi, min(len(self.pool), self.hi + fresh)
        rows = [self.pool[i] for i in rng.integers(0, max(self.hi, 1), size=n).tolist()]
        new = self.pool[lo:self.hi][:n]                                    # every new entry of the window is fed, among rows drawn from all of it
        for at, r in zip(rng.permutation(n)[:len(new)].tolist(), new):
            rows[at] = r
        self.n_retired = 0
        if self.retired and n:
            for at in rng.integers(0, n, size=max(1, n // 10)).tolist():
                rows[at] = self.retired[int(rng.integers(len(self.retired)))][1]
                self.n_retired += 1
        return rows

    def form(self, n):
        rng = self.rng
        mem = str(rng.choice(["host", "device"]))
        return {"bits": int(rng.choice([32, 64])), "validity": bool(rng.random() < 0.4), "mem": mem, "voff": int(rng.integers(0, 9)),
                "shift": int(rng.integers(1, 16)) if mem == "device" and rng.random() < 0.6 else 0}

    def batch(self, kind, rows_a, rows_b=None, **more):
        rng, n = self.rng, len(rows_a)
        sides = 2 if rows_b is not None else 1
        op = dict(kind=kind, n=n, sides=sides, ints=[{}, {}], strs=[{}, {}], forms={}, str_max_new={}, keep_a=None, keep_b=None, max_new=None,
                  key_mem=str(rng.choice(["host", "device"])))
        for s, rows in enumerate((rows_a, rows_b)[:sides]):
            for c in range(self.n_cols):
                col = [r[c] for r in rows]
                if c in self.str_cols:
                    f = op["forms"][(c, s)] = self.form(n)
                    op["strs"][s][c] = (col, (rng.random(n) < 0.1) if f["validity"] else None)
                    op["str_max_new"][(c, s)] = int(rng.integers(0, 4)) if rng.random() < 0.2 else None
                else:
                    op["ints"][s][c] = np.array(col, I64)
        if rng.random() < 0.35:
            op["keep_a"] = (rng.random(n) < 0.8).astype(U8)
        if sides == 2 and rng.random() < 0.35:
            op["keep_b"] = (rng.random(n) < 0.8).astype(U8)
        op.update(more)
        return op

    def two_sided(self):
        return self.cls == "wide" or (self.cls in ("long", "collide") and self.rng.random() < 0.3)

    def encode(self, n=None, fresh=None, first_rows=()):
        rng = self.rng
        n = int(rng.integers(self.rows[0], self.rows[1] + 1)) if n is None else n
        fresh = int(n * rng.choice([0.3, 0.6, 0.9])) if fresh is None else fresh
        two = self.two_sided() and not first_rows
        rows_a = list(first_rows) + self.draw_rows(n - len(first_rows), fresh)
        rows_b = self.draw_rows(n, fresh // 2) if two else None
        op = self.batch("encode", rows_a, rows_b)
        if first_rows:                         # the engineered rows come first, whole and in order
            op["keep_a"] = None
            for k in op["forms"]:
                op["forms"][k]["validity"] = False
                op["strs"][k[1]][k[0]] = (op["strs"][k[1]][k[0]][0], None)
        return op

    def cap_new(self, op):
        """a max_new below the number of new keys, in some batches: decided on a copy of the model"""
        if self.rng.random() < 0.3:
            probe = DictSetModel(self.n_cols, self.str_cols)
            probe.vocabs = [VocabModel(v.values) for v in self.m.vocabs]
            probe.keys = KeyDictModel(self.n_cols, self.m.keys.keys)
            before = len(probe.keys)
            apply(probe, op)
            new = len(probe.keys) - before
            if new > 1:
                op["max_new"] = int(self.rng.integers(0, new))
        return op

    def lookup(self, n=None):
        rng = self.rng
        n = int(rng.integers(8, 65)) if n is None else n
        hi, self.hi = self.hi, min(len(self.pool), self.hi + n)          # some never fed ...
        rows_a = self.draw_rows(n, 0)
        rows_b = self.draw_rows(n, 0) if rng.random() < (0.8 if self.cls == "wide" else 0.3) else None
        self.hi = hi                                                        # ... and the window stays
        held = self.m.raw_keys()
        if held:                                                            # and some held for certain
            for at in rng.integers(0, n, size=max(1, n // 3)).tolist():
                rows_a[at] = held[int(rng.integers(len(held)))][1]
        return self.batch("lookup", rows_a, rows_b, retired_rows=self.n_retired)

    # -- patterns, from the values themselves --
    def some_value(self, v, limit=48):
        vals = self.m.vocabs[v].values or self.strings[v]
        s = vals[int(self.rng.integers(len(vals)))]
        if len(s) > limit:
            at = int(self.rng.integers(0, len(s) - limit + 1))
            s = s[at:at + limit]
        return s

    def swap_case(self, s):
        return bytes((b ^ 0x20) if (0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A) and self.rng.random() < 0.5 else b for b in s)

    def like_pattern(self, v, nocase):
        rng = self.rng
        whole = rng.random() < 0.4
        s = self.some_value(v, 1 << 20 if whole else 48)
        if len(s) > 400:
            s, whole = s[:400], False
        out = bytearray()
        for b in (self.swap_case(s) if nocase else s):
            r = rng.random()
            if r < 0.08:
                out += b"_" if not 0x80 <= b <= 0xBF else b""
            elif r < 0.11:
                out += b"%"
            elif b in b"%_\\" or r < 0.15:
                out += b"\\" + bytes([b])
            else:
                out.append(b)
        if not whole or rng.random() < 0.5:
            out = (b"%" if rng.random() < 0.8 else b"") + out + (b"%" if rng.random() < 0.8 else b"")
        return bytes(out)

    def term(self, col):
        rng, v = self.rng, self.str_cols[col]
        how = str(rng.choice(["equal", "contains", "like", "like"]))
        if how == "equal":
            return dict(col=col, how="match", op=STR_EQUAL, pattern=self.some_value(v, MAX_PATTERN), nocase=False)
        if how == "contains":
            s = self.some_value(v, 12)
            return dict(col=col, how="match", op=STR_CONTAINS_NOCASE, pattern=self.swap_case(s[: max(1, len(s) // 2)]), nocase=True)
        nocase = bool(rng.random() < 0.5)
        return dict(col=col, how="like", op=None, pattern=self.like_pattern(v, nocase), nocase=nocase)

    def select(self):
        rng = self.rng
        cols = sorted(self.str_cols)
        terms = [self.term(cols[int(rng.integers(len(cols)))]) for _ in range(int(rng.integers(1, 4)))]
        return dict(kind="select", terms=terms, side=[None, 0, 1][int(rng.integers(3))], mem=str(rng.choice(["host", "device"])))

    def like(self):
        rng = self.rng
        v = int(rng.integers(len(self.m.vocabs)))
        nocase = bool(rng.random() < 0.5)
        return dict(kind="like", vocab=v, pattern=self.like_pattern(v, nocase), nocase=nocase, mem=str(rng.choice(["host", "device"])))

    def decode(self):
        rng, K = self.rng, len(self.m.keys)
        n = int(rng.integers(1, 200)) if K else 0
        ids = rng.integers(0, max(K, 1), size=n).astype(U64)
        if self.cls == "long" and K:            # the heavy values are few: ask for the keys that hold them
            heavy = [i for i, (_, t) in enumerate(self.m.raw_keys()) if len(t[1]) >= 4095]
            ids = np.concatenate([ids[:40], np.array(heavy[:int(rng.integers(0, 6))] * 2, U64)])
            rng.shuffle(ids)
        cols = None
        if rng.random() < 0.4:
            cols = sorted(rng.choice(self.n_cols, size=int(rng.integers(1, self.n_cols + 1)), replace=False).tolist())
        mem = str(rng.choice(["host", "device"]))
        return dict(kind="decode", ids=ids, cols=cols, mem=mem, strings_to="host" if mem == "host" or rng.random() < 0.5 else "device")

    def restart(self):
        return dict(kind="restart", slices=int(self.rng.choice([1, 7, 100, 1000])) if self.seed % 2 else None)

    def compact_keys(self, variant=None, share=None):
        rng, K = self.rng, len(self.m.keys)
        if K == 0:                             # nothing to compact: feed the dictionaries instead
            return self.cap_new(self.encode())
        if variant is None:                    # a script's first drawn compaction takes the survivor set its seed names
            self.compactions += 1
            variant = SURVIVORS[self.seed % len(SURVIVORS)] if self.compactions == 1 else str(rng.choice(SURVIVORS, p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.1]))
        alive = np.zeros(K, bool)
        if variant == "share":
            alive = rng.random(K) < (share if share is not None else float(rng.choice([0.1, 0.5, 0.9])))
        elif variant == "all":
            alive[:] = True
        elif variant == "prefix":
            alive[: max(int(K * (share if share is not None else 0.3)), min(K, 40))] = True
        elif variant == "last":
            alive[K - 1:] = True
        elif variant == "but_first":
            alive[1:] = True
        return dict(kind="compact_keys", remap=survivors_remap(alive), mem=str(rng.choice(["host", "device"])), variant=variant)

    def retire_strings(self, superset=None):
        rng, extras = self.rng, []
        superset = rng.random() < 0.4 if superset is None else superset
        for voc in self.m.vocabs:
            n = len(voc)
            extras.append(np.unique(rng.integers(0, n, size=int(rng.integers(1, 6)))) if superset and n else np.zeros(0, I64))
        return dict(kind="retire_strings", extras=extras, mem=str(rng.choice(["host", "device"])), superset=bool(superset))

    def refused(self):
        rng, m = self.rng, self.m
        start = (self.seed + 5 * self.refusals) % len(REFUSALS)
        self.refusals += 1
        for k in range(len(REFUSALS)):
            op = self.refusal(REFUSALS[(start + k) % len(REFUSALS)])
            if op is not None:
                return op
        raise AssertionError("no refusal applies")

    def refusal(self, variant):
        """the arguments of one refusal, or None where the model does not hold what it needs"""
        rng, m = self.rng, self.m
        K, keys = len(m.keys), m.keys.keys
        op = dict(kind="refused", variant=variant)
        cols = sorted(self.str_cols)
        col = cols[int(rng.integers(len(cols)))]
        v = self.str_cols[col]
        voc = m.vocabs[v]
        if variant.startswith("remap_"):
            if K < 4:
                return None
            alive = rng.random(K) < 0.7
            alive[:3] = True
            remap = survivors_remap(alive)
            if variant == "remap_swapped":
                remap[[0, 1]] = remap[[1, 0]]
            elif variant == "remap_duplicate":
                remap[2] = remap[1]
            elif variant == "remap_gap":
                remap[alive] += (np.arange(int(alive.sum())) >= 2).astype(U64)
            else:
                remap = np.concatenate([remap, [U64(alive.sum())]]) if rng.random() < 0.5 else remap[:-1]
            op.update(remap=remap.astype(U64), mem=str(rng.choice(["host", "device"])))
        elif variant == "recode_to_none":
            if not K:
                return None
            remap = np.arange(len(voc), dtype=I64)
            remap[keys[int(rng.integers(K))][1][col]] = CODE_NONE
            op.update(remaps=[(col, remap)], mem=str(rng.choice(["host", "device"])))
        elif variant == "recode_makes_equal":
            def alike(c):                     # two keys that differ in column c alone
                rest = [(s, t[:c] + t[c + 1:]) for s, t in keys]
                return len(set(rest)) < len(rest)
            col = next((c for c in [col] + cols if alike(c)), None)
            if col is None:
                return None
            voc = m.vocabs[self.str_cols[col]]
            op.update(remaps=[(col, np.zeros(len(voc), I64))], mem=str(rng.choice(["host", "device"])))
        elif variant == "column_twice":
            ident = np.arange(len(voc), dtype=I64)
            op.update(remaps=[(col, ident), (col, ident.copy())], mem=str(rng.choice(["host", "device"])))
        elif variant == "stale_keep_len":
            op.update(vocab=v, keep=np.ones(len(voc) + (1 if len(voc) == 0 or rng.random() < 0.5 else -1), U8), mem=str(rng.choice(["host", "device"])))
        elif variant in ("match_stale_mask_len", "like_stale_mask_len"):
            op.update(vocab=v, mask_len=len(voc) + (1 if len(voc) == 0 or rng.random() < 0.5 else -1), pattern=b"%a%" if "like" in variant else b"a",
                      mem=str(rng.choice(["host", "device"])))
        elif variant == "import_nonempty":
            target = "keys" if K and rng.random() < 0.5 else "values"
            if target == "values" and not len(voc):
                return None
            op.update(target=target, vocab=v, load=([np.arange(2, dtype=I64) + 5 for _ in range(self.n_cols)], np.zeros(2, U8)) if target == "keys"
                      else [b"one", b"two"])
        elif variant == "import_duplicate":
            target = str(rng.choice(["keys", "values"]))
            if target == "keys":
                c = [np.array([3, 4, 5, 4, 6], I64) for _ in range(self.n_cols)]
                op.update(target=target, vocab=v, load=(c, np.array([0, 1, 0, 1, 0], U8)))
            else:
                op.update(target=target, vocab=v, load=[b"a", b"", b"bb", b"a" * 40, b"", b"c"])
        elif variant == "offsets_decrease":
            new = [b"never-seen-%d-%d" % (self.seed, i) for i in range(5)]
            strings = new + [self.some_value(v) + b"#" for _ in range(20)]
            off, data = arrow(strings)
            off[-2] = off[-1] + 1 if rng.random() < 0.3 else off[-2]      # (beyond data_bytes and then decreasing) ...
            off[-3] = off[-2] + 3                                          # ... or decreasing alone, in a late row
            op.update(vocab=v, offsets=off.astype(np.int32) if rng.random() < 0.5 else off, data=data, mem=str(rng.choice(["host", "device"])))
        elif variant == "gather_num_keys":
            ids = rng.integers(0, max(K, 1), size=9).astype(U64)
            ids[int(rng.integers(9))] = K
            op.update(ids=ids, mem=str(rng.choice(["host", "device"])))
        elif variant == "decode_num_values":
            codes = rng.integers(0, max(len(voc), 1), size=9).astype(I64)
            codes[int(rng.integers(9))] = len(voc)
            op.update(vocab=v, codes=codes, mem=str(rng.choice(["host", "device"])))
        elif variant == "mark_used_len_below":
            top = max((t[col] for _, t in keys), default=0)
            if top < 1:
                return None
            op.update(col=col, used_len=top, mem=str(rng.choice(["host", "device"])))
        return op

    # -- the read-only checks after an operation --
    def checks(self):
        second = str(self.rng.choice(CHECK_KINDS))
        return [self.lookup(), getattr(self, second)()]

    # -- the script --
    def plan(self):
        rng = self.rng
        if self.cls == "churn":
            kinds = ["encode_big", "encode_big", "compact_hard", "retire_strings", "encode_past", "restart", "encode", "compact_hard", "retire_strings",
                     "encode_past", "refused", str(rng.choice(KINDS))]
            return kinds
        kinds = [str(rng.choice(KINDS, p=[0.3, 0.06, 0.1, 0.1, 0.08, 0.11, 0.11, 0.14])) for _ in range(N_OPS)]
        if self.cls == "collide":
            kinds[:4] = ["encode_engineered", "encode_grow", "compact_prefix", "retire_strings"]
        elif self.seed % 4:
            kinds[0] = "encode"                # one script in four starts on the empty dictionaries with whatever was drawn
        if self.cls == "growth":               # growth after a compaction, of the table, the records and the arena
            kinds[3:7] = ["encode", "compact_hard", "retire_strings", "encode_past"]
        if "refused" not in kinds:
            kinds[-1 - self.seed % 3] = "refused"
        return kinds

    def engineered_rows(self):
        (pa, pb), cluster = collide_tuples()
        (sa, sb), scluster = collide_strings()
        rows = [(7, ANCHOR)] + [(x, ANCHOR) for x in (pa, pb) + cluster]
        return rows + [(8 + i, s) for i, s in enumerate((sa, sb) + tuple(scluster))]

    def draw(self, kind):
        if kind == "encode_engineered":
            rows = self.engineered_rows()
            return self.encode(n=len(rows) + 6, fresh=6, first_rows=rows)
        if kind == "encode_grow":
            return self.encode(n=260, fresh=240)
        if kind == "encode_big":
            return self.encode(n=self.rows[1], fresh=int(self.rows[1] * 0.9))
        if kind == "encode_past":              # past the old maximum of keys and values
            need = max(self.max_keys - len(self.m.keys), 0) + 300
            n = min(need + 200, 3000 if self.cls == "growth" else 1 << 20)
            op = self.encode(n=n, fresh=n)
            op["keep_a"] = None                # every row takes part
            return op
        if kind == "compact_hard":
            return self.compact_keys("share", 0.15)
        if kind == "compact_prefix":
            return self.compact_keys("prefix", 0.3)
        if kind == "encode":
            return self.cap_new(self.encode())
        if kind == "retire_to_zero":
            return self.retire_strings(superset=False)
        return getattr(self, kind)()

    def account(self, op, out, before):
        """what the operation does to the documented capacities -> info for the coverage assertions"""
        m = self.m
        info = {"keys_before": before[0], "values_before": before[1], "keys_after": len(m.keys), "values_after": [len(v) for v in m.vocabs], "grew": [],
                "grew_after_compaction": []}
        kind = op["kind"]

        def note(caps, what, grew):
            for g in grew:
                info["grew"].append(what + "_" + g)
                if caps.compacted:
                    info["grew_after_compaction"].append(what + "_" + g)

        if kind == "encode":
            for v, voc in enumerate(m.vocabs):
                note(self.sd_caps[v], "values", self.sd_caps[v].reserve(len(voc), voc.padded()))
            note(self.kd_caps, "keys", self.kd_caps.reserve(len(m.keys)))
        elif kind == "restart":
            self.kd_caps = _Caps(self.expected[0])
            self.kd_caps.reserve(len(m.keys))
            self.sd_caps = [_Caps(self.expected[1], self.expected[2]) for _ in m.vocabs]
            for v, voc in enumerate(m.vocabs):
                self.sd_caps[v].reserve(len(voc), voc.padded())
        elif kind == "compact_keys":
            self.kd_caps.compact(before[0], len(m.keys))
        elif kind == "retire_strings":
            for v, voc in enumerate(m.vocabs):
                self.sd_caps[v].compact(before[1][v], len(voc), voc.padded())
        return info

    def script(self):
        ops, kinds = [], self.plan()
        for at, kind in enumerate(kinds):
            m = self.m
            if ops and ops[-1]["kind"] == "compact_keys" and ops[-1]["info"]["keys_before"] and not len(m.keys):
                kind = "retire_to_zero"        # every key went: the chain then empties the vocabularies
            op = self.draw(kind)
            before = (len(m.keys), [len(v) for v in m.vocabs])
            held = m.raw_keys() if op["kind"] == "compact_keys" else None
            lengths = sorted({len(s) for v in m.vocabs for s in v.values})
            out = apply(m, op)
            op["info"] = self.account(op, out, before)
            op["info"]["lengths_held"] = lengths
            if held is not None:
                gone = [k for k, r in zip(held, op["remap"].tolist()) if r == int(KEY_SKIP)]
                self.retired = (self.retired + gone)[-400:]
            self.max_keys, self.max_values = max(self.max_keys, len(m.keys)), max(self.max_values, max(len(v) for v in m.vocabs))
            op["info"].update(max_keys=self.max_keys, max_values=self.max_values)
            op["checks"] = self.checks()
            for ch in op["checks"]:
                ch["info"] = {"lengths_held": sorted({len(s) for v in m.vocabs for s in v.values})}
            ops.append(op)
        return ops


def make_script(seed):
    """-> {"seed", "class", "n_cols", "str_cols", "expected", "ops"}: a function of the seed alone"""
    g = _Gen(seed)
    ops = g.script()
    return {"seed": seed, "class": g.cls, "n_cols": g.n_cols, "str_cols": dict(g.str_cols), "expected": g.expected, "ops": ops}


def new_model(sc):
    return DictSetModel(sc["n_cols"], sc["str_cols"])


def describe(op):
    """an operation without its columns, for assertion messages"""
    out = {}
    for k, x in op.items():
        if k in ("checks", "info", "ints", "strs"):
            continue
        if isinstance(x, np.ndarray):
            x = "array%s%s" % (x.shape, x[:6].tolist())
        elif isinstance(x, (list, tuple)) and len(x) > 8:
            x = "%s[%d]" % (type(x).__name__, len(x))
        elif isinstance(x, bytes) and len(x) > 80:
            x = x[:80] + b"...(%d)" % len(x)
        out[k] = x
    return out
