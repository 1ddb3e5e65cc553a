"""CPU tests of the string dictionary's boundary (include/tad.h: TAD_FEATURE_STRING_DICT and the tad_strdict_* calls): the feature bit and the
prototypes in the header, the ctypes mirror, the exported symbols, tad_features() without a device, the Python wrapper's behaviour
against a library without the bit, and the Go binding's guard.  No compute calls."""
import ctypes
import inspect
import os
import re

import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_strdict_create": ("int", ["tad_engine *e", "uint64_t expected_values", "uint64_t expected_bytes", "tad_strdict **out"]),
    "tad_strdict_destroy": ("void", ["tad_engine *e", "tad_strdict *d"]),
    "tad_strdict_encode": ("int", ["tad_engine *e", "tad_strdict *d", "const tad_string_column *col", "int64_t *codes", "uint64_t *new_first_row",
                                   "uint64_t new_first_row_cap", "uint64_t *num_before", "uint64_t *num_values"]),
    "tad_strdict_lookup": ("int", ["tad_engine *e", "const tad_strdict *d", "const tad_string_column *col", "int64_t *codes"]),
    "tad_strdict_num_values": ("int", ["tad_engine *e", "const tad_strdict *d", "uint64_t *num_values"]),
    "tad_strdict_bytes": ("int", ["tad_engine *e", "const tad_strdict *d", "uint64_t *bytes"]),
    "tad_strdict_export": ("int", ["tad_engine *e", "const tad_strdict *d", "uint64_t first_code", "uint64_t n_values", "int64_t *offsets", "uint8_t *data",
                                   "uint64_t data_cap", "uint64_t *data_bytes"]),
    "tad_strdict_import": ("int", ["tad_engine *e", "tad_strdict *d", "uint64_t n_values", "const int64_t *offsets", "const uint8_t *data"]),
    "tad_strdict_match": ("int", ["tad_engine *e", "const tad_strdict *d", "int32_t op", "const uint8_t *pattern", "uint64_t pattern_len", "uint8_t *mask",
                                  "uint64_t mask_len", "tad_mem memory", "uint64_t *n_matched"]),
}
GO_METHODS = {      # the Go function that binds each call
    "tad_strdict_create": "func (e *Engine) NewStringDict(", "tad_strdict_destroy": "func (d *StringDict) Close(", "tad_strdict_encode": "func (d *StringDict) Encode(",
    "tad_strdict_lookup": "func (d *StringDict) Lookup(", "tad_strdict_num_values": "func (d *StringDict) NumValues(", "tad_strdict_bytes": "func (d *StringDict) Bytes(",
    "tad_strdict_export": "func (d *StringDict) Export(", "tad_strdict_import": "func (d *StringDict) Import(", "tad_strdict_match": "func (d *StringDict) Match(",
}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STRING_DICT\s+4096u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    assert re.search(r"#define\s+TAD_CODE_NONE\s+\(-1\)", HEADER)
    assert re.search(r"#define\s+TAD_STR_EQUAL\s+0\b", HEADER) and re.search(r"#define\s+TAD_STR_CONTAINS_NOCASE\s+1\b", HEADER)
    assert re.search(r"typedef struct tad_strdict tad_strdict;", CODE)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_documents_the_contract_in_front_of_the_calls():
    start = HEADER.index("TAD_FEATURE_STRING_DICT; check tad_features()")
    assert HEADER.index("int tad_drop_state_keys(") < start < HEADER.index("int tad_strdict_create(") < HEADER.index("int tad_progress(")
    section = HEADER[start:HEADER.index("int tad_strdict_create(")]
    for must in ("FIRST APPEARANCE", "new_first_row", "tad_encode_strings", "never reused", "TAD_CODE_NONE", "before the dictionary is touched", "EMPTY",
                 "TAD_ERR_GRID_TOO_LARGE", "size query", "stale length is refused", "'A'..'Z'", ">= 0x80", "Kubernetes", "ilike", "tad_keydict_select",
                 "workspace_limit", "tad_strdict_bytes", "Lock order: the dictionary, then a job context"):
        assert must in section, must


def test_ctypes_symbols_and_the_constants():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STRING_DICT == 4096 and _capi.TAD_ABI_VERSION == 13 and _capi.TAD_CODE_NONE == -1
    assert (_capi.TAD_STR_EQUAL, _capi.TAD_STR_CONTAINS_NOCASE) == (0, 1)
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args), name
        assert res is (None if name == "tad_strdict_destroy" else ctypes.c_int), name
    assert _capi.SYMBOLS["tad_strdict_encode"][1][2] == ctypes.POINTER(_capi.StringColumn)
    assert _capi.SYMBOLS["tad_strdict_create"][1][1:3] == [ctypes.c_uint64, ctypes.c_uint64]
    assert ctypes.sizeof(_capi.StringColumn) == 64 and ctypes.sizeof(_capi.KeyColumns) == 56      # no existing struct grew


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 4096 and f & _capi.TAD_FEATURE_STRING_DICT
    assert f & 4095 == 4095                                                                 # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    out = ctypes.c_void_p(7)
    assert lib.tad_strdict_create(None, 0, 0, ctypes.byref(out)) == inv and out.value == 7
    a, b = ctypes.c_uint64(5), ctypes.c_uint64(6)
    assert lib.tad_strdict_encode(None, None, None, None, None, 0, ctypes.byref(a), ctypes.byref(b)) == inv and (a.value, b.value) == (5, 6)
    assert lib.tad_strdict_lookup(None, None, None, None) == inv
    assert lib.tad_strdict_num_values(None, None, ctypes.byref(a)) == inv and a.value == 5
    assert lib.tad_strdict_bytes(None, None, ctypes.byref(a)) == inv and a.value == 5
    assert lib.tad_strdict_export(None, None, 0, 0, None, None, 0, ctypes.byref(a)) == inv and a.value == 5
    assert lib.tad_strdict_import(None, None, 0, None, None) == inv
    mask = (ctypes.c_ubyte * 4)(9, 9, 9, 9)
    assert lib.tad_strdict_match(None, None, 0, None, 0, ctypes.cast(mask, ctypes.c_void_p), 4, 0, ctypes.byref(a)) == inv and a.value == 5 and list(mask) == [9] * 4
    lib.tad_strdict_destroy(None, None)                                                     # a no-op


def test_the_unit_is_hip_in_its_own_source():
    from theia_amd import build
    assert "tad_strdict.hip" in build.SOURCES and "tad_capi_strdict.cpp" in build.SOURCES
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    src = open(os.path.join(csrc, "tad_strdict.hip")).read()
    for name in ("k_sd_probe", "k_sd_append", "k_sd_fix", "k_sd_rehash", "k_sd_match", "k_sd_export", "launch_sd_probe", "launch_sd_append", "launch_sd_rehash",
                 "launch_sd_match", "atomicCAS"):
        assert name in src, name
    assert not re.search(r"\basm\b|__asm", src) and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert includes == ["tad_internal.h", "tad_strbytes.h"]                                 # project-internal headers only
    assert all(os.path.exists(os.path.join(csrc, h)) for h in includes)
    # the byte helpers live in the shared header, and tad_encode_strings' file uses them from there; the column they read (StrBatch: what StrArgs and
    # SdBatch were) lives in tad_internal.h, where the host side fills it
    shared = open(os.path.join(csrc, "tad_strbytes.h")).read()
    fz = open(os.path.join(csrc, "tad_factorize.hip")).read()
    assert "struct StrBatch" in open(os.path.join(csrc, "tad_internal.h")).read() and "struct StrBatch" not in fz and "struct StrArgs" not in fz
    for name in ("bool se_span(", "uint64_t se_load(", "uint64_t se_load_lds(", "uint64_t se_hash(", "bool se_same_as("):
        assert name in shared and name not in fz, name
    assert '#include "tad_strbytes.h"' in fz


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("StringDict touched %s on a library without TAD_FEATURE_STRING_DICT" % name)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        raise AssertionError("no call may be made")


def test_string_dict_raises_cleanly_without_the_feature_bit():
    from theia_amd import StringDict, TadEngine, TadError, _capi
    with pytest.raises(TadError) as ei:
        StringDict(_FakeEngine(_FakeLib(4095)))
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STRING_DICT" in ei.value.message

    class NoFeatures:                   # older still: not even tad_features
        pass
    with pytest.raises(TadError) as ei:
        StringDict(_FakeEngine(NoFeatures()))
    assert "TAD_FEATURE_STRING_DICT" in ei.value.message
    sig = inspect.signature(TadEngine.string_dict)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("self", inspect.Parameter.empty), ("expected_values", 0), ("expected_bytes", 0)]
    for method in ("encode", "lookup", "num_values", "nbytes", "values", "load", "match", "close"):
        assert callable(getattr(StringDict, method)), method


def test_go_binding_binds_every_call_behind_its_guard():
    assert "func hasStringDict() bool" in GO and "C.tad_features()&C.TAD_FEATURE_STRING_DICT" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        if name != "tad_strdict_destroy":                                                   # (closing needs no question: the handle came from the library)
            assert body.index("hasStringDict()") < body.index("C.%s(" % name), name
    # the struct handed to C lives in C memory, and so does everything it points to: no Go pointer is stored in it
    sb = GO[GO.index("func stringBatch("):]
    sb = sb[:sb.index("\n}\n")]
    assert "C.calloc(1, C.size_t(unsafe.Sizeof(C.tad_string_column{})))" in sb and "C.CBytes(" in sb
    assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", sb)
