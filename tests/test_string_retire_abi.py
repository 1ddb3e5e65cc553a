"""CPU tests of the boundary of retiring dead strings (include/tad.h: TAD_FEATURE_STRING_RETIRE, tad_keydict_mark_codes,
tad_strdict_compact, tad_keydict_recode): the feature bit, the prototypes and the stats struct in the header, where the section stands and
what it says, the ctypes mirror, the exported symbols, tad_features() and the NULL-engine refusals without a device, the kernels' source,
the Python wrappers against a library without the bit, the Go binding's guard and the Python signatures.  No compute calls."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_keydict_mark_codes": ("int", ["tad_engine *e", "const tad_keydict *d", "int32_t col", "int32_t accumulate", "uint8_t *used", "uint64_t used_len",
                                       "tad_mem memory", "uint64_t *n_used"]),
    "tad_strdict_compact": ("int", ["tad_engine *e", "tad_strdict *d", "const uint8_t *keep", "uint64_t keep_len", "tad_mem keep_memory", "int64_t *remap",
                                    "tad_mem remap_memory", "tad_strdict_compact_stats *stats"]),
    "tad_keydict_recode": ("int", ["tad_engine *e", "tad_keydict *d", "int32_t n_terms", "const int32_t *term_col", "const int64_t *const *remaps",
                                   "const uint64_t *remap_len", "tad_mem memory", "uint64_t *num_keys"]),
}
STATS_FIELDS = [("uint64_t", "values_before"), ("uint64_t", "values_after"), ("uint64_t", "bytes_before"), ("uint64_t", "bytes_after"),
                ("uint64_t", "arena_used_before"), ("uint64_t", "arena_used_after"), ("int32_t", "job_context"), ("int32_t", "reserved"), ("float", "ms_total"),
                ("float", "reserved1")]
GO_METHODS = {"tad_keydict_mark_codes": "func (d *KeyDict) UsedCodes(", "tad_strdict_compact": "func (d *StringDict) Compact(",
              "tad_keydict_recode": "func (d *KeyDict) Recode("}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STRING_RETIRE\s+16384u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_declares_the_stats_struct_field_for_field():
    body = re.search(r"typedef struct \{([^}]*)\}\s*tad_strdict_compact_stats;", CODE, flags=re.S)
    assert body, "tad_strdict_compact_stats is not declared"
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            typ, names = decl.split(" ", 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    assert fields == STATS_FIELDS


def test_header_documents_the_contract_between_the_decode_and_the_progress_calls():
    start = HEADER.index("TAD_FEATURE_STRING_RETIRE; check tad_features()")
    assert HEADER.index("int tad_strdict_decode(") < start < HEADER.index("int tad_keydict_mark_codes(") < HEADER.index("int tad_strdict_compact(") \
        < HEADER.index("int tad_keydict_recode(") < HEADER.index("int tad_progress(")
    section = " ".join(HEADER[start:HEADER.index("#define TAD_FEATURE_STRING_RETIRE")].replace("\n *", " ").split())     # the comment's text, unwrapped
    for must in ("accumulate", "either side", "used is unspecified", "refused before anything runs", "An empty dictionary is TAD_OK", "stale length is refused",
                 "never a short read", "number of survivors below it", "first appearance", "TAD_CODE_NONE", "m, m + 1", "expected_values = 2 m",
                 "tad_strdict_bytes never grows", "packed", "16-byte aligned", "zero-padded", "swapped in last", "TAD_ERR_GRID_TOO_LARGE", "workspace_limit",
                 "remap is the identity", "nothing is reallocated or moved", "m == 0", "LDS", "a column named twice", "recoded tuples are equal",
                 "n_terms == 0", "NEW codes", "old id", "The ABI version does not change and no struct grows",
                 "Lock order: the dictionary, then a job context", "tools/strdict_retire_bench.py"):
        assert must in section, must
    # the section quotes no earlier prototype, and every "...; check tad_features()" phrase stays unique: the older tests find theirs by the first occurrence
    assert not re.search(r"\bint tad_\w+\(", section)
    for other in re.findall(r"TAD_FEATURE_\w+; check tad_features\(\)", HEADER):
        assert HEADER.count(other) == 1, other
    # the two dictionaries' own sections name the new exception to "never moved", and keep what they said
    sd = HEADER[HEADER.index("TAD_FEATURE_STRING_DICT; check tad_features()"):HEADER.index("int tad_strdict_create(")]
    assert "Codes are never reused or moved." in sd and "tad_strdict_compact" in sd
    kd = HEADER[HEADER.index("TAD_FEATURE_KEY_DICT; check tad_features()"):HEADER.index("int tad_keydict_create(")]
    assert "never" in kd and "tad_keydict_compact" in kd and "tad_keydict_recode" in kd


def test_ctypes_symbols_the_feature_constant_and_the_struct_against_gcc(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STRING_RETIRE == 16384 and _capi.TAD_ABI_VERSION == 13
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args) and res is ctypes.c_int, name
    assert _capi.SYMBOLS["tad_keydict_mark_codes"][1][2:4] == [ctypes.c_int32, ctypes.c_int32] and _capi.SYMBOLS["tad_keydict_mark_codes"][1][5] == ctypes.c_uint64
    assert _capi.SYMBOLS["tad_strdict_compact"][1][3] == ctypes.c_uint64 and _capi.SYMBOLS["tad_strdict_compact"][1][7] == ctypes.POINTER(_capi.StrdictCompactStats)
    assert _capi.SYMBOLS["tad_keydict_recode"][1][4] == ctypes.POINTER(ctypes.c_void_p) and _capi.SYMBOLS["tad_keydict_recode"][1][5] == ctypes.POINTER(ctypes.c_uint64)
    assert [n for n, _ in _capi.StrdictCompactStats._fields_] == [n for _, n in STATS_FIELDS]
    assert ctypes.sizeof(_capi.StrdictCompactStats) == 64
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.KeyColumns, _capi.StringColumn, _capi.CompactStats, _capi.MergeStats)] == [136, 96, 56, 64, 96, 104]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(tad_strdict_compact_stats), '
                   'offsetof(tad_strdict_compact_stats, arena_used_after), offsetof(tad_strdict_compact_stats, job_context), '
                   'offsetof(tad_strdict_compact_stats, ms_total)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    S = _capi.StrdictCompactStats
    assert [int(x) for x in out] == [ctypes.sizeof(S), S.arena_used_after.offset, S.job_context.offset, S.ms_total.offset]


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 16384 and f & _capi.TAD_FEATURE_STRING_RETIRE
    assert f & 16383 == 16383                                                               # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    used = np.full(8, 0x5A, dtype=np.uint8)
    n = ctypes.c_uint64(77)
    for mem in (_capi.TAD_MEM_HOST, _capi.TAD_MEM_DEVICE):
        assert lib.tad_keydict_mark_codes(None, None, 0, 0, used.ctypes.data, 8, mem, ctypes.byref(n)) == inv
        assert lib.tad_keydict_mark_codes(None, None, 0, 1, used.ctypes.data, 8, mem, None) == inv
    assert (used == 0x5A).all() and n.value == 77
    keep = np.ones(4, dtype=np.uint8)
    remap = np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    cs = _capi.StrdictCompactStats(values_before=5, values_after=6, bytes_after=7)
    assert lib.tad_strdict_compact(None, None, keep.ctypes.data, 4, _capi.TAD_MEM_HOST, remap.ctypes.data, _capi.TAD_MEM_HOST, ctypes.byref(cs)) == inv
    assert lib.tad_strdict_compact(None, None, None, 0, _capi.TAD_MEM_DEVICE, None, _capi.TAD_MEM_DEVICE, None) == inv
    assert (remap == 0x5A5A5A5A5A5A5A5A).all() and (cs.values_before, cs.values_after, cs.bytes_after) == (5, 6, 7)
    cols = (ctypes.c_int32 * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(remap.ctypes.data)
    lens = (ctypes.c_uint64 * 1)(4)
    assert lib.tad_keydict_recode(None, None, 1, cols, ptrs, lens, _capi.TAD_MEM_HOST, ctypes.byref(n)) == inv
    assert lib.tad_keydict_recode(None, None, 0, None, None, None, _capi.TAD_MEM_DEVICE, None) == inv
    assert n.value == 77


def test_the_kernels_are_hip_in_the_dictionaries_own_units():
    from theia_amd import build
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    assert "tad_keydict.hip" in build.SOURCES and "tad_strdict.hip" in build.SOURCES
    kd = open(os.path.join(csrc, "tad_keydict.hip")).read()
    sd = open(os.path.join(csrc, "tad_strdict.hip")).read()
    for name in ("k_kd_mark", "k_kd_count_used", "k_kd_recode", "launch_kd_mark", "launch_kd_count_used", "launch_kd_recode", "block_count_add(s_cnt, n_used",
                 "kd_load_record(keys, k, pairs, w)"):
        assert name in kd, name
    for name in ("k_sd_compact_flags", "k_sd_compact_recs", "k_sd_compact_copy", "k_sd_compact_rehash", "launch_sd_compact_copy", "kSdCopyLaneMax", "slot_claim(table, mask"):
        assert name in sd, name
    copy = sd[sd.index("void k_sd_compact_copy("):sd.index("void k_sd_compact_rehash(")]
    assert "__shared__" in copy and "uint4" in copy and "__syncthreads()" in copy        # the offsets in LDS, whole 16-byte words
    for src in (kd, sd):
        assert not re.search(r"\basm\b|__asm", src) and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", kd) == ["tad_internal.h", "tad_slots.h"]
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", sd) == ["tad_internal.h", "tad_strbytes.h"]
    # the entry points sit with their dictionaries' host sides; candidates are filled first and committed last
    khost = open(os.path.join(csrc, "tad_capi_keydict.cpp")).read()
    assert "int tad_keydict_mark_codes(" in khost and "int tad_keydict_recode(" in khost
    body = khost[khost.index("int tad_keydict_recode("):]
    assert body.index("launch_kd_recode(") < body.index("launch_kd_rehash(") < body.index("KD_FLAG_DUPLICATE") < body.index("commit_into(")
    shost = open(os.path.join(csrc, "tad_capi_strdict.cpp")).read()
    body = shost[shost.index("int tad_strdict_compact("):]
    assert body.index("over_limit(") < body.index("launch_sd_compact_flags(") < body.index("launch_scan(") < body.index("launch_sd_compact_recs(s, w.live, w.newcode, w.off16, d->recs, K, d_remap, nrecs.p") \
        < body.index("launch_sd_compact_copy(") < body.index("launch_sd_compact_rehash(") < body.index("commit_into(")


class _FakeLib:
    """a library of before the feature: every earlier bit, and none of the three calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def tad_keydict_create(self, eng, n_cols, expected, out):
        return 0

    def tad_strdict_create(self, eng, values, nbytes, out):
        return 0

    def tad_keydict_destroy(self, eng, h):
        pass

    def tad_strdict_destroy(self, eng, h):
        pass

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STRING_RETIRE" % name)


class _NoFeatures:
    tad_keydict_create = tad_strdict_create = staticmethod(lambda *a: 0)
    tad_keydict_destroy = tad_strdict_destroy = staticmethod(lambda *a: None)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        assert rc == 0


def test_the_wrappers_raise_cleanly_without_the_feature_bit():
    from theia_amd import KeyDict, StringDict, TadError, _capi
    from theia_amd.stream_detection import StreamingAnomalyDetection
    eng = _FakeEngine(_FakeLib(16383))
    kd, sd = KeyDict(eng, 2), StringDict(eng)                     # the constructors still succeed
    calls = [lambda: kd.used_codes(0, 4), lambda: kd.used_codes(0, 4, into=np.zeros(4, np.uint8), out="host"), lambda: sd.compact(np.ones(4, np.uint8)),
             lambda: kd.recode({0: np.arange(4)}), lambda: kd.recode({})]
    sad = StreamingAnomalyDetection.__new__(StreamingAnomalyDetection)
    sad._engine, sad._dict, sad._vocab, sad._state, sad._broken = eng, kd, [sd], None, None
    calls.append(sad.retire)
    for call in calls:
        with pytest.raises(TadError) as ei:
            call()
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STRING_RETIRE" in ei.value.message
    # a library of before tad_features
    old = _FakeEngine(_NoFeatures())
    kd = KeyDict.__new__(KeyDict)
    kd._engine, kd._h, kd.n_cols = old, None, 1
    with pytest.raises(TadError) as ei:
        kd.recode({0: np.arange(2)})
    assert "TAD_FEATURE_STRING_RETIRE" in ei.value.message


def test_go_binding_binds_the_three_calls_behind_its_guard():
    assert "func hasStringRetire() bool" in GO and "C.tad_features()&C.TAD_FEATURE_STRING_RETIRE" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        assert body.index("hasStringRetire()") < body.index("C.%s(" % name), name
        # the arrays cross in C memory: no pointer into a Go slice is handed to the library
        assert ("C.calloc(" in body or "C.malloc(" in body or "cColumn(" in body) and "C.free(" in body, name
        assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", body), name
    assert "never compiled" in GO[GO.index("func hasStringRetire() bool") - 1500:GO.index("func hasStringRetire() bool")]


def test_the_python_methods_have_the_documented_signatures():
    from theia_amd import KeyDict, StringDict
    from theia_amd.stream_detection import StreamingAnomalyDetection

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(KeyDict.used_codes) == [("self", E), ("col", E), ("n_values", E), ("into", None), ("out", "device")]
    assert sig(StringDict.compact) == [("self", E), ("keep", E), ("out", "host")]
    assert sig(KeyDict.recode) == [("self", E), ("remaps", E)]
    assert sig(StreamingAnomalyDetection.retire) == [("self", E), ("idle_before", 0)]
    doc = " ".join(StreamingAnomalyDetection.retire.__doc__.split())
    assert "NOT consistent" in doc and "snapshot" in doc and "before the first vocabulary is compacted" in doc
