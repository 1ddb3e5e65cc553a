"""CPU tests of the key dictionary's boundary (include/tad.h: TAD_FEATURE_KEY_DICT and the tad_keydict_* calls): the feature bit and the
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
    "tad_keydict_create": ("int", ["tad_engine *e", "int32_t n_cols", "uint64_t expected_keys", "tad_keydict **out"]),
    "tad_keydict_destroy": ("void", ["tad_engine *e", "tad_keydict *d"]),
    "tad_keydict_encode": ("int", ["tad_engine *e", "tad_keydict *d", "const tad_key_columns *kc", "uint64_t *key_id", "uint64_t *key_id2",
                                   "uint64_t *new_first_row", "uint64_t new_first_row_cap", "uint64_t *num_keys_before", "uint64_t *num_keys"]),
    "tad_keydict_lookup": ("int", ["tad_engine *e", "const tad_keydict *d", "const tad_key_columns *kc", "uint64_t *key_id", "uint64_t *key_id2"]),
    "tad_keydict_num_keys": ("int", ["tad_engine *e", "const tad_keydict *d", "uint64_t *num_keys"]),
    "tad_keydict_bytes": ("int", ["tad_engine *e", "const tad_keydict *d", "uint64_t *bytes"]),
    "tad_keydict_export": ("int", ["tad_engine *e", "const tad_keydict *d", "uint64_t first_key", "uint64_t n_keys", "int64_t *const *cols", "uint8_t *side"]),
    "tad_keydict_import": ("int", ["tad_engine *e", "tad_keydict *d", "uint64_t n_keys", "const int64_t *const *cols", "const uint8_t *side"]),
}
GO_METHODS = {      # the Go function that binds each call
    "tad_keydict_create": "func (e *Engine) NewKeyDict(", "tad_keydict_destroy": "func (d *KeyDict) Close(", "tad_keydict_encode": "func (d *KeyDict) Encode(",
    "tad_keydict_lookup": "func (d *KeyDict) Lookup(", "tad_keydict_num_keys": "func (d *KeyDict) NumKeys(", "tad_keydict_bytes": "func (d *KeyDict) Bytes(",
    "tad_keydict_export": "func (d *KeyDict) Export(", "tad_keydict_import": "func (d *KeyDict) Import(",
}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_KEY_DICT\s+128u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    assert re.search(r"typedef struct tad_keydict tad_keydict;", CODE)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_documents_the_contract_in_front_of_the_calls():
    start = HEADER.index("TAD_FEATURE_KEY_DICT; check tad_features()")
    assert HEADER.index("int tad_run_state_window(") < start < HEADER.index("int tad_keydict_create(") < HEADER.index("int tad_progress(")
    section = HEADER[start:HEADER.index("int tad_keydict_create(")]
    for must in ("first appearance", "TAD_KEY_SKIP", "new_first_row", "tad_factorize", "never", "EMPTY", "workspace_limit", "tad_keydict_bytes",
                 "Lock order: the dictionary, then a job context"):
        assert must in section, must


def test_ctypes_symbols_and_the_feature_constant():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_KEY_DICT == 128 and _capi.TAD_ABI_VERSION == 13
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args), name
        assert res is (None if name == "tad_keydict_destroy" else ctypes.c_int), name
    assert _capi.SYMBOLS["tad_keydict_encode"][1][2] == ctypes.POINTER(_capi.KeyColumns)
    assert _capi.SYMBOLS["tad_keydict_create"][1][1:3] == [ctypes.c_int32, ctypes.c_uint64]
    assert ctypes.sizeof(_capi.KeyColumns) == 56 and ctypes.sizeof(_capi.Columns) == 96      # no existing struct grew


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 128 and f & _capi.TAD_FEATURE_KEY_DICT
    assert f & 127 == 127                                                                   # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    out = ctypes.c_void_p(7)
    assert lib.tad_keydict_create(None, 2, 0, ctypes.byref(out)) == _capi.TAD_ERR_INVALID_ARGUMENT and out.value == 7
    assert lib.tad_keydict_encode(None, None, None, None, None, None, 0, None, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_keydict_lookup(None, None, None, None, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    n = ctypes.c_uint64(5)
    assert lib.tad_keydict_num_keys(None, None, ctypes.byref(n)) == _capi.TAD_ERR_INVALID_ARGUMENT and n.value == 5
    assert lib.tad_keydict_export(None, None, 0, 0, None, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_keydict_import(None, None, 0, None, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    lib.tad_keydict_destroy(None, None)                                                     # a no-op


def test_the_unit_is_hip_in_its_own_source():
    from theia_amd import build
    assert "tad_keydict.hip" in build.SOURCES and "tad_capi_keydict.cpp" in build.SOURCES
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_keydict.hip")).read()
    for name in ("k_kd_probe", "k_kd_append", "k_kd_fix", "k_kd_rehash", "launch_kd_probe", "launch_kd_append", "launch_kd_rehash", "atomicCAS"):
        assert name in src, name
    assert "asm" not in src and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src) == ["tad_internal.h", "tad_slots.h"]


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("KeyDict touched %s on a library without TAD_FEATURE_KEY_DICT" % name)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        raise AssertionError("no call may be made")


def test_key_dict_raises_cleanly_without_the_feature_bit():
    from theia_amd import KeyDict, TadEngine, TadError, _capi
    with pytest.raises(TadError) as ei:
        KeyDict(_FakeEngine(_FakeLib(127)), 3)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_KEY_DICT" in ei.value.message

    class NoFeatures:                   # older still: not even tad_features
        pass
    with pytest.raises(TadError) as ei:
        KeyDict(_FakeEngine(NoFeatures()), 3)
    assert "TAD_FEATURE_KEY_DICT" in ei.value.message
    sig = inspect.signature(TadEngine.key_dict)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("self", inspect.Parameter.empty), ("n_cols", inspect.Parameter.empty), ("expected_keys", 0)]
    for method in ("encode", "lookup", "num_keys", "nbytes", "export", "load", "close"):
        assert callable(getattr(KeyDict, method)), method


def test_go_binding_binds_every_call_behind_its_guard():
    assert "func hasKeyDict() bool" in GO and "C.tad_features()&C.TAD_FEATURE_KEY_DICT" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        if name != "tad_keydict_destroy":                                                   # (closing needs no question: the handle came from the library)
            assert body.index("hasKeyDict()") < body.index("C.%s(" % name), name
    # the struct handed to C lives in C memory, and so does everything it points to: no Go pointer is stored in it
    kb = GO[GO.index("func keyBatch("):]
    kb = kb[:kb.index("\n}\n")]
    assert "C.calloc(1, C.size_t(unsafe.Sizeof(C.tad_key_columns{})))" in kb and "cColumn(col)" in kb and "C.CBytes(m)" in kb
    assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", kb)
