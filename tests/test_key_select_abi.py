"""CPU tests of the boundary of the key-filtered state jobs (include/tad.h: TAD_FEATURE_KEY_SELECT, tad_keydict_select,
tad_run_state_keys, tad_drop_state_keys): the feature bit, the exact prototypes and what the section's text promises, a C snippet against
the header, the ctypes mirror, the exported symbols, tad_features() and the NULL refusals without a device, the kernels' source, the
Python wrappers against a library without the bit, the Go binding's guard.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

KEYS_ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "int64_t from_t", "int64_t to_t", "uint64_t keep_points", "const uint8_t *key_keep",
             "uint64_t key_keep_len", "tad_mem key_memory", "tad_mem out_memory", "tad_result **out"]
PROTOTYPES = {
    "tad_keydict_select": ("int", ["tad_engine *e", "const tad_keydict *d", "int32_t n_terms", "const int32_t *term_col", "const uint8_t *const *masks",
                                   "const uint64_t *mask_len", "int32_t side", "uint8_t *key_keep", "uint64_t key_keep_len", "tad_mem memory",
                                   "uint64_t *n_selected"]),
    "tad_run_state_keys": ("int", KEYS_ARGS),
    "tad_drop_state_keys": ("int", KEYS_ARGS),
}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_KEY_SELECT\s+2048u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_section_names_the_contract():
    start = HEADER.index("TAD_FEATURE_KEY_SELECT; check tad_features()")
    assert HEADER.index("void tad_drop_rows_free(") < start < HEADER.index("int tad_keydict_select(") < HEADER.index("int tad_run_state_keys(") \
        < HEADER.index("int tad_drop_state_keys(") < HEADER.index("int tad_progress(")
    section = " ".join(HEADER[start:HEADER.index("#define TAD_FEATURE_KEY_SELECT")].replace("\n *", " ").split())     # the comment's text, unwrapped
    for must in ("--pod-name", "--svc-port-name", "KEY selections", "masks[t][tuple_k[term_col[t]]] != 0", "tad_mask_rows' rule", "0 .. 8",
                 "a stale length is refused", "raised from a device flag", "key_keep is then unspecified", "The dictionary is never changed",
                 "Lock order: the dictionary, then a job context", "whose key has key_keep[key] != 0", "exactly the rows tad_run returns for W''",
                 "nothing is renumbered", "is the window call itself", "any non-zero byte selects", "An empty selection is TAD_OK with zero rows",
                 "the state is bit for bit what it was", "rows_in = rows_used = n_points", "costs no fit", "the all-zero-window shortcut is not taken",
                 "tad_window_history_by_sort with the SELECTED window points", "Lock order: the state, then a job context"):
        assert must in section, must


def test_ctypes_mirror_the_calls_and_a_c_snippet_compiles_against_the_header(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_KEY_SELECT == 2048 and _capi.TAD_ABI_VERSION == 13
    vp, u64, i64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32
    assert _capi.SYMBOLS["tad_keydict_select"] == (ctypes.c_int, [vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(u64), i32, vp, u64,
                                                                  ctypes.c_int, ctypes.POINTER(u64)])
    keys = (ctypes.c_int, [vp, vp, ctypes.POINTER(_capi.Job), i64, i64, u64, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.POINTER(_capi.Result))])
    assert _capi.SYMBOLS["tad_run_state_keys"] == keys and _capi.SYMBOLS["tad_drop_state_keys"] == keys
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns)] == [136, 96]                       # no existing struct grew
    src = tmp_path / "use.c"
    src.write_text('#include <stdio.h>\n#include "tad.h"\n'
                   'static int pick(tad_engine *e, tad_keydict *d, tad_state *s, const tad_job *job, uint64_t n) {\n'
                   '  const uint8_t web[4] = {0, 1, 0, 0};\n  const uint8_t *const masks[1] = {web};\n  const int32_t col[1] = {1};\n'
                   '  const uint64_t len[1] = {4};\n  static uint8_t keep[16];\n  uint64_t picked = 0;\n  tad_result *r = NULL;\n'
                   '  int rc = tad_keydict_select(e, d, 1, col, masks, len, -1, keep, n, TAD_MEM_HOST, &picked);\n'
                   '  if (rc == TAD_OK) rc = tad_run_state_keys(e, s, job, 0, 0, 0, keep, n, TAD_MEM_HOST, TAD_MEM_HOST, &r);\n'
                   '  if (rc == TAD_OK) rc = tad_drop_state_keys(e, s, job, 0, 0, 0, NULL, 0, TAD_MEM_HOST, TAD_MEM_DEVICE, &r);\n  return rc;\n}\n'
                   'int main(void) { printf("%u %d %zu %zu\\n", TAD_FEATURE_KEY_SELECT, TAD_ABI_VERSION, sizeof(tad_job), sizeof(tad_columns)); '
                   '(void)pick; return 0; }\n')
    obj = tmp_path / "use.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(obj), str(src)], check=True)
    size = tmp_path / "size.c"
    size.write_text('#include <stdio.h>\n#include "tad.h"\nint main(void) { printf("%u %d %zu %zu\\n", TAD_FEATURE_KEY_SELECT, TAD_ABI_VERSION, '
                    'sizeof(tad_job), sizeof(tad_columns)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(size)], check=True)
    assert [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [2048, 13, 136, 96]


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 2048 and f & 4095 == 4095                                                    # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    bad = _capi.TAD_ERR_INVALID_ARGUMENT
    keep = np.zeros(4, np.uint8)
    n_sel = ctypes.c_uint64(77)
    # a NULL engine is refused without a device, with a message, and nothing is written
    assert lib.tad_keydict_select(None, None, 0, None, None, None, -1, keep.ctypes.data, 4, _capi.TAD_MEM_HOST, ctypes.byref(n_sel)) == bad
    assert b"tad_keydict_select: engine is NULL" in lib.tad_last_error(None) and n_sel.value == 77
    job = _capi.Job()
    res = ctypes.POINTER(_capi.Result)()
    for name in ("tad_run_state_keys", "tad_drop_state_keys"):
        fn = getattr(lib, name)
        assert fn(None, None, ctypes.byref(job), 0, 0, 0, keep.ctypes.data, 4, _capi.TAD_MEM_HOST, _capi.TAD_MEM_HOST, ctypes.byref(res)) == bad
        assert ("%s: engine is NULL" % name).encode() in lib.tad_last_error(None)
        assert fn(None, None, None, 0, 0, 0, None, 0, _capi.TAD_MEM_HOST, _capi.TAD_MEM_HOST, None) == bad
        assert not res


def test_the_kernels_are_hip_in_the_units_the_design_names():
    from theia_amd import build
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    assert "tad_keydict.hip" in build.SOURCES and "tad_window.hip" in build.SOURCES
    kd = open(os.path.join(csrc, "tad_keydict.hip")).read()
    assert "k_kd_select" in kd and "launch_kd_select" in kd and "asm" not in kd and "rocprim" not in kd.lower()
    assert "launch_kd_select" in open(os.path.join(csrc, "tad_capi_keydict.cpp")).read()
    host = open(os.path.join(csrc, "tad_capi_view.cpp")).read()
    assert "int tad_run_state_keys(" in host and "int tad_drop_state_keys(" in host
    assert "TAD_FEATURE_KEY_SELECT" in open(os.path.join(csrc, "tad_engine.cpp")).read()


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("a wrapper touched %s on a library without TAD_FEATURE_KEY_SELECT" % name)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, None


@pytest.mark.parametrize("lib", [_FakeLib(2047), object()], ids=["without-the-bit", "without-tad_features"])
def test_the_wrappers_raise_cleanly_without_the_feature_bit(lib):
    from theia_amd import KeyDict, TadEngine, TadError, _capi
    from theia_amd.engine import TadState
    eng = TadEngine.__new__(TadEngine)
    eng._lib, eng._h = lib, None
    st = TadState.__new__(TadState)
    st._engine, st._h, st.num_keys = eng, None, 4
    keep = np.ones(4, np.uint8)
    d = KeyDict.__new__(KeyDict)
    d._engine, d._h, d.n_cols = _FakeEngine(lib), None, 2
    for call in (lambda: eng.run_state_keys(st, keep), lambda: eng.drop_state_keys(st, keep), lambda: d.select([(0, keep)]),
                 lambda: d.select([], side=1, out="host")):
        with pytest.raises(TadError) as ei:
            call()
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_KEY_SELECT" in ei.value.message
    st._h = d._h = None                                        # nothing to free


def test_go_binding_binds_the_calls_behind_their_guard():
    assert "func hasKeySelect() bool" in GO and "C.tad_features()&C.TAD_FEATURE_KEY_SELECT" in GO
    for fn, call in (("func (d *KeyDict) Select(", "C.tad_keydict_select("), ("func (s *State) RunKeys(", "C.tad_run_state_keys("),
                     ("func (s *State) DropKeys(", "C.tad_drop_state_keys(")):
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert body.index("hasKeySelect()") < body.index(call), fn
    sel = GO[GO.index("func (d *KeyDict) Select("):]
    sel = sel[:sel.index("\n}\n")]
    assert "var pin runtime.Pinner" in sel and "defer pin.Unpin()" in sel and sel.index("pin.Pin(&t.Mask[0])") < sel.index("C.tad_keydict_select(")


def test_the_host_layers_exist():
    import inspect
    from theia_amd import KeyDict, TadEngine
    assert list(inspect.signature(KeyDict.select).parameters) == ["self", "terms", "side", "out"]
    sig = inspect.signature(TadEngine.run_state_keys)
    assert list(sig.parameters)[:6] == ["self", "state", "key_keep", "from_t", "to_t", "keep_points"] and sig.parameters["algo"].default == "EWMA"
    assert list(inspect.signature(TadEngine.drop_state_keys).parameters)[:6] == ["self", "state", "key_keep", "from_t", "to_t", "keep_points"]
