"""What drives a KeyDict and the StringDicts of its string columns next to their host model (tests/dict_model.py): one operation of a
script executed on the engine (`execute`, `run_check` for the read-only ones), the whole content (`snapshot`), and the comparison of a
call's outputs with the model's (`assert_outputs`).  No test in this module."""
import ctypes as C

import numpy as np

import dict_model as dm
from job_helpers import column, device_column
from theia_amd import TadError
from theia_amd import _capi as capi
from theia_amd.engine import DeviceArray

U64, I64, U8 = np.uint64, np.int64, np.uint8
STAT_FIELDS = ("values_before", "values_after", "arena_used_before", "arena_used_after")


class Dicts:
    """one key dictionary and the vocabularies of its string columns"""

    def __init__(self, engine, sc):
        self.sc = sc
        ek, ev, eb = sc["expected"]
        self.kd = engine.key_dict(sc["n_cols"], expected_keys=ek)
        self.sd = [engine.string_dict(expected_values=ev, expected_bytes=eb) for _ in range(1 + max(sc["str_cols"].values()))]

    def vocab_of(self, col):
        return self.sd[self.sc["str_cols"][col]]

    def nbytes(self):
        return [self.kd.nbytes()] + [d.nbytes() for d in self.sd]

    def close(self):
        self.kd.close()
        for d in self.sd:
            d.close()


def new_dicts(engine, sc):
    return Dicts(engine, sc)


def values_of(d):
    off, data = d.export()
    raw = data.tobytes()
    assert off[0] == 0 and off.size == d.num_values() + 1, ("export", off[:1], off.size)
    return [raw[off[i]:off[i + 1]] for i in range(off.size - 1)]


def snapshot(dicts):
    """the whole content, in the form DictSetModel.snapshot gives it"""
    cols, side = dicts.kd.export()
    return {"num_keys": dicts.kd.num_keys(), "key_cols": cols, "key_side": side, "num_values": [d.num_values() for d in dicts.sd],
            "values": [values_of(d) for d in dicts.sd]}


def assert_snapshot(got, want, what):
    assert got["num_keys"] == want["num_keys"], (what, "num_keys", got["num_keys"], want["num_keys"])
    assert got["num_values"] == want["num_values"], (what, "num_values", got["num_values"], want["num_values"])
    for c, (g, w) in enumerate(zip(got["key_cols"], want["key_cols"])):
        same(g, w, (what, "key column", c))
    same(got["key_side"], want["key_side"], (what, "key sides"))
    for v, (g, w) in enumerate(zip(got["values"], want["values"])):
        if g != w:
            at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            raise AssertionError((what, "vocabulary", v, "first difference at value", at, g[at:at + 1], w[at:at + 1]))


def host(x):
    return x.to_host() if isinstance(x, DeviceArray) else np.asarray(x)


def same(got, want, what):
    """bit for bit: the same type, length and bytes"""
    got, want = host(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError((what, "first difference at", at, got[at:at + 4].tolist(), want[at:at + 4].tolist(), "of", got.size))


def device_bytes(engine, a):
    """a uint8 array as a DeviceArray of its bytes"""
    a = np.ascontiguousarray(a, U8)
    d = DeviceArray.from_host(engine, np.frombuffer(a.tobytes() + b"\0" * (-a.size % 8 or (8 if a.size == 0 else 0)), dtype=U64))
    return d.view(0, a.size, U8)


def to_mem(engine, a, mem):
    if mem == "host":
        return a
    return device_bytes(engine, a) if a.dtype == U8 else DeviceArray.from_host(engine, a if a.size else np.zeros(1, a.dtype)).view(0, a.size, a.dtype)


def string_column(engine, strings, nulls, form):
    """the column in the Arrow form the script drew: offset width, validity bitmap (whose nulls still own bytes), memory, byte shift"""
    valid = None if nulls is None else ~nulls
    if form["mem"] == "device":
        return device_column(engine, strings, form["bits"], form["shift"], valid, form["voff"] if valid is not None else 0)
    off, data = column(strings, form["bits"])
    if valid is None:
        return off, data
    bits = np.concatenate([np.ones(form["voff"], bool), valid])
    return off, data, np.packbits(bits, bitorder="little"), form["voff"]


def key_columns(engine, dicts, op, codes):
    """the tuple columns of both sides in op["key_mem"]: the int columns as drawn, the string columns as the codes the vocabularies gave"""
    sides = []
    for s in range(op["sides"]):
        cols = []
        for c in range(dicts.sc["n_cols"]):
            x = codes[(c, s)] if c in dicts.sc["str_cols"] else op["ints"][s][c]
            if op["key_mem"] == "device" and not isinstance(x, DeviceArray):
                x = DeviceArray.from_host(engine, x if x.size else np.zeros(1, I64))
                x.n = op["n"]
            cols.append(x)
        sides.append(cols)
    return sides[0], (sides[1] if op["sides"] == 2 else None)


def batch(engine, dicts, op):
    """an encode or a lookup: every string column through its vocabulary (by column, side a before side b), then the tuples"""
    kind = op["kind"]
    codes, out = {}, {"str": []}
    for c, s in [(c, s) for c in sorted(dicts.sc["str_cols"]) for s in range(op["sides"])]:
        strings, nulls = op["strs"][s][c]
        form = op["forms"][(c, s)]
        col = string_column(engine, strings, nulls if form["validity"] else None, form)
        d = dicts.vocab_of(c)
        if kind == "encode":
            cd, first, before = d.encode(col, out=op["key_mem"], max_new=op["str_max_new"][(c, s)])
            out["str"].append({"codes": host(cd), "first": host(first), "before": before, "after": d.num_values()})
        else:
            cd = d.lookup(col, out=op["key_mem"])
            out["str"].append({"codes": host(cd)})
        codes[(c, s)] = cd
    a, b = key_columns(engine, dicts, op, codes)
    if kind == "encode":
        k1, k2, first, before = dicts.kd.encode(a, op["keep_a"], b, op["keep_b"], max_new=op["max_new"])
        out.update(key1=host(k1), key2=None if k2 is None else host(k2), first=host(first), before=before)
    else:
        k1, k2 = dicts.kd.lookup(a, op["keep_a"], b, op["keep_b"])
        out.update(key1=host(k1), key2=None if k2 is None else host(k2))
    out["num_keys"] = dicts.kd.num_keys()
    return out


def select(engine, dicts, op):
    masks, terms = [], []
    for t in op["terms"]:
        d = dicts.vocab_of(t["col"])
        m, n = d.like(t["pattern"], nocase=t["nocase"], out=op["mem"]) if t["how"] == "like" else d.match(t["op"], t["pattern"], out=op["mem"])
        masks.append((host(m), n))
        terms.append((t["col"], m))
    keep, n = dicts.kd.select(terms, side=op["side"], out=op["mem"])
    return {"masks": masks, "keep": host(keep), "n_selected": n}


def decode(engine, dicts, op):
    ids = op["ids"]
    if op["mem"] == "device":
        ids = DeviceArray.from_host(engine, ids if ids.size else np.zeros(1, U64))
        ids.n = op["ids"].size
    columns, side = dicts.kd.gather(ids, op["cols"], out=op["mem"])
    want = list(range(dicts.sc["n_cols"])) if op["cols"] is None else op["cols"]
    decoded = {}
    for c, col in zip(want, columns):
        if c in dicts.sc["str_cols"]:
            off, data = dicts.vocab_of(c).decode(col, out=op["strings_to"])       # (device codes may give host strings)
            decoded[c] = (host(off), host(data))
    return {"columns": [host(c) for c in columns], "side": host(side), "decoded": decoded}


def restart(engine, dicts, op):
    """export both kinds (in slices for some seeds), close, fresh objects, load: the host restarted -> (the fresh dictionaries, what was exported)"""
    K, step = dicts.kd.num_keys(), op["slices"]
    if step is None:
        cols, side = dicts.kd.export()
        values = [d.export() for d in dicts.sd]
    else:
        parts = [dicts.kd.export(f, min(step, K - f)) for f in range(0, K, step)] or [dicts.kd.export()]
        cols = [np.concatenate([p[0][c] for p in parts]) for c in range(dicts.sc["n_cols"])]
        side = np.concatenate([p[1] for p in parts])
        values = []
        for d in dicts.sd:
            n = d.num_values()
            vp = [d.export(f, min(step, n - f)) for f in range(0, n, step)] or [d.export()]
            off = np.concatenate([np.zeros(1, I64)] + [p[0][1:] + sum(int(q[0][-1]) for q in vp[:i]) for i, p in enumerate(vp)])
            values.append((off, np.concatenate([p[1] for p in vp])))
    raw = [v[1].tobytes() for v in values]
    exported = {"num_keys": K, "key_cols": cols, "key_side": side, "num_values": [v[0].size - 1 for v in values],
                "values": [[r[v[0][i]:v[0][i + 1]] for i in range(v[0].size - 1)] for v, r in zip(values, raw)]}
    sc = dicts.sc
    dicts.close()
    fresh = Dicts(engine, sc)
    fresh.kd.load(cols, side)
    for d, v in zip(fresh.sd, values):
        d.load(v)
    return fresh, {"exported": exported}


def retire_strings(engine, dicts, op):
    """the chain: per vocabulary one mark call per column that shares it (accumulating from the second on), one compact, then ONE recode"""
    sc, mem = dicts.sc, op["mem"]
    out = {"n_used": {}, "used": {}, "remaps": {}, "stats": {}}
    remaps = {}
    for v, d in enumerate(dicts.sd):
        used, counts, n_values = None, [], d.num_values()
        for c in [c for c in sorted(sc["str_cols"]) if sc["str_cols"][c] == v]:
            used, n = dicts.kd.used_codes(c, n_values, into=used, out=mem)
            counts.append(n)
        keep = used
        if op["extras"][v].size:                                   # a superset: extra values the host wants kept
            keep = host(used).copy()
            keep[op["extras"][v]] = 1
            keep = to_mem(engine, keep, mem)
        remap, stats = d.compact(keep, out=mem)
        remaps[v] = remap
        out["n_used"][v], out["used"][v], out["remaps"][v] = counts, host(used), host(remap)
        out["stats"][v] = {f: stats[f] for f in STAT_FIELDS}
        out.setdefault("bytes", {})[v] = (stats["bytes_before"], stats["bytes_after"])
    try:
        out["num_keys"] = dicts.kd.recode({c: remaps[sc["str_cols"][c]] for c in sorted(sc["str_cols"])})
    except TadError as exc:                # (wrong marks end here: the masks and counts above are compared first and name the call)
        out["num_keys"] = ("recode refused", str(exc))
    return out


def raw_mask_call(engine, d, op):
    """tad_strdict_match / tad_strdict_like with a mask_len of the caller's (the wrappers always pass num_values)"""
    K, pat = op["mask_len"], op["pattern"]
    buf = (C.c_ubyte * len(pat)).from_buffer_copy(pat)
    dev = op["mem"] == "device"
    mask = device_bytes(engine, np.zeros(K, U8)) if dev else np.zeros(max(K, 1), U8)
    ptr = mask.ptr if dev else mask.ctypes.data
    mem = capi.TAD_MEM_DEVICE if dev else capi.TAD_MEM_HOST
    hit, lib = capi.u64(), engine._lib
    if op["variant"] == "match_stale_mask_len":
        rc = lib.tad_strdict_match(engine._h, d._h, dm.STR_CONTAINS_NOCASE, C.cast(buf, C.c_void_p), len(pat), ptr, K, mem, C.byref(hit))
    else:
        rc = lib.tad_strdict_like(engine._h, d._h, C.cast(buf, C.c_void_p), len(pat), 0, ptr, K, mem, C.byref(hit))
    engine._check(rc)


def refused_call(engine, dicts, op):
    v, mem = op["variant"], op.get("mem", "host")
    if v.startswith("remap_"):
        dicts.kd.compact(to_mem(engine, op["remap"], mem))
    elif v in ("recode_to_none", "recode_makes_equal", "column_twice"):
        dicts.kd.recode([(c, to_mem(engine, r, mem)) for c, r in op["remaps"]])
    elif v == "stale_keep_len":
        dicts.sd[op["vocab"]].compact(to_mem(engine, op["keep"], mem))
    elif v in ("match_stale_mask_len", "like_stale_mask_len"):
        raw_mask_call(engine, dicts.sd[op["vocab"]], op)
    elif v == "import_nonempty":
        if op["target"] == "keys":
            dicts.kd.load(*op["load"])
        else:
            dicts.sd[op["vocab"]].load(op["load"])
    elif v == "import_duplicate":                                  # a fresh dictionary refuses it, and stays empty
        d = engine.key_dict(dicts.sc["n_cols"], expected_keys=1) if op["target"] == "keys" else engine.string_dict(1, 1)
        try:
            d.load(*op["load"]) if op["target"] == "keys" else d.load(op["load"])
        finally:
            left = d.num_keys() if op["target"] == "keys" else d.num_values()
            d.close()
            assert left == 0, ("a refused import left", left)
    elif v == "offsets_decrease":
        col = (op["offsets"], op["data"])
        if mem == "device":
            col = (DeviceArray.from_host(engine, op["offsets"]), device_bytes(engine, op["data"]))
        dicts.sd[op["vocab"]].encode(col)
    elif v == "gather_num_keys":
        dicts.kd.gather(to_mem(engine, op["ids"], mem), out=mem)
    elif v == "decode_num_values":
        dicts.sd[op["vocab"]].decode(to_mem(engine, op["codes"], mem))
    elif v == "mark_used_len_below":
        dicts.kd.used_codes(op["col"], op["used_len"], out=mem)
    else:
        raise ValueError(v)


def execute(engine, dicts, sc, op):
    """one operation of a script on the dictionaries -> (the dictionaries, the call's own outputs in the form dict_model.apply gives them)"""
    kind = op["kind"]
    if kind in ("encode", "lookup"):
        return dicts, batch(engine, dicts, op)
    if kind == "select":
        return dicts, select(engine, dicts, op)
    if kind == "like":
        m, n = dicts.sd[op["vocab"]].like(op["pattern"], nocase=op["nocase"], out=op["mem"])
        return dicts, {"mask": host(m), "n_matched": n}
    if kind == "decode":
        return dicts, decode(engine, dicts, op)
    if kind == "restart":
        return restart(engine, dicts, op)
    if kind == "compact_keys":
        return dicts, {"num_keys": dicts.kd.compact(to_mem(engine, op["remap"], op["mem"]))}
    if kind == "retire_strings":
        return dicts, retire_strings(engine, dicts, op)
    if kind == "refused":
        try:
            refused_call(engine, dicts, op)
        except TadError:
            return dicts, {"raises": True}
        return dicts, {"raises": False}
    raise ValueError(kind)


def run_check(engine, dicts, sc, check):
    """a read-only operation: the dictionaries are the same objects afterwards"""
    same_dicts, out = execute(engine, dicts, sc, check)
    assert same_dicts is dicts
    return out


def assert_outputs(got, want, tag):
    """a call's own outputs against the model's, bit for bit; for a refusal only that it was refused"""
    if "raises" in want:
        assert got.get("raises"), (tag, "the call must be refused")
        return
    got = {k: v for k, v in got.items() if k != "bytes"}
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if key == "str":
            assert len(g) == len(w), (tag, key)
            for j, (gs, ws) in enumerate(zip(g, w)):
                assert set(gs) == set(ws), (tag, key, j)
                for f in ws:
                    (same(gs[f], ws[f], (tag, "string step", j, f)) if isinstance(ws[f], np.ndarray) else _eq(gs[f], ws[f], (tag, "string step", j, f)))
        elif key == "masks":
            assert len(g) == len(w), (tag, key)
            for j, ((gm, gn), (wm, wn)) in enumerate(zip(g, w)):
                same(gm, wm, (tag, "mask of term", j))
                _eq(gn, wn, (tag, "n_matched of term", j))
        elif key == "columns":
            assert len(g) == len(w), (tag, key)
            for j, (gc, wc) in enumerate(zip(g, w)):
                same(gc, wc, (tag, "gathered column", j))
        elif key == "decoded":
            assert set(g) == set(w), (tag, key, sorted(g), sorted(w))
            for c in w:
                same(g[c][0], w[c][0], (tag, "decoded offsets of column", c))
                same(g[c][1], w[c][1], (tag, "decoded bytes of column", c))
        elif key == "exported":
            assert_snapshot(g, w, (tag, "exported"))
        elif key in ("used", "remaps"):
            for v in w:
                same(g[v], w[v], (tag, key, "vocabulary", v))
        elif key in ("n_used", "stats"):
            _eq(g, w, (tag, key))
        elif w is None or not isinstance(w, np.ndarray):
            _eq(g, w, (tag, key))
        else:
            same(g, w, (tag, key))


def _eq(got, want, what):
    assert got == want, (what, got, want)
