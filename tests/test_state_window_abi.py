"""CPU tests of tad_run_state_window's boundary (include/tad.h): the feature bit and the prototype in the header and where they sit, the
ctypes mirror, the exported symbol, tad_features() without a device, the Python method's defaults and the Go binding's guard.  No compute
calls."""
import ctypes
import inspect
import os
import re
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_WINDOW\s+64u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


def test_header_declares_the_call_with_its_exact_arguments():
    proto = re.search(r"int\s+tad_run_state_window\s*\(([^;]*?)\)\s*;", CODE, flags=re.S)
    assert proto, "tad_run_state_window is not declared"
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    assert args == ["tad_engine *e", "tad_state *s", "const tad_job *job", "int64_t from_t", "int64_t to_t", "uint64_t keep_points",
                    "tad_mem out_memory", "tad_result **out"]


def test_header_section_sits_between_the_merge_and_the_progress_calls():
    assert CODE.index("int tad_state_merge(") < CODE.index("TAD_FEATURE_STATE_WINDOW") < CODE.index("int tad_run_state_window(") \
        < CODE.index("int tad_progress(")
    assert HEADER.index("int tad_state_merge(") < HEADER.index("TAD_FEATURE_STATE_WINDOW; check tad_features()") < HEADER.index("int tad_progress(")
    section = HEADER[HEADER.index("TAD_FEATURE_STATE_WINDOW; check tad_features()"):HEADER.index("int tad_run_state_window(")]
    assert "flowStartSeconds" in section and "tad_state_bytes" in section      # the caveat of from_t; the workspace is not the state's


def test_ctypes_symbol_entry_and_struct_sizes():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_WINDOW == 64 and _capi.TAD_ABI_VERSION == 13
    res, args = _capi.SYMBOLS["tad_run_state_window"]
    assert res is ctypes.c_int and len(args) == 8
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_capi.Job), ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int,
                    ctypes.POINTER(ctypes.POINTER(_capi.Result))]
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136      # no existing struct grew


def test_library_exports_the_symbol_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_run_state_window")
    f = lib.tad_features()
    assert f & 64 and f & _capi.TAD_FEATURE_STATE_WINDOW
    assert f & (1 | 2 | 4 | 8 | 16 | 32) == 63                                         # every earlier bit is still set
    assert lib.tad_abi_version() == 13


def test_python_method_signature():
    from theia_amd.engine import TadEngine
    got = [(p.name, p.default) for p in inspect.signature(TadEngine.run_state_window).parameters.values()]
    E = inspect.Parameter.empty
    assert got == [("self", E), ("state", E), ("from_t", 0), ("to_t", 0), ("keep_points", 0), ("algo", "EWMA"), ("alpha", 0.0), ("eps", 0.0),
                   ("min_samples", 0), ("maxiter", 0), ("emit_all", False), ("out", "host"), ("job_id", "")]
    run = inspect.signature(TadEngine.run_state).parameters
    for name, default in got[1:]:
        if name in run:
            assert run[name].default == default, name       # shared parameters keep run_state's defaults


def test_go_binding_asks_the_library_before_using_the_call():
    assert "func hasStateWindow() bool" in GO and "C.tad_features()&C.TAD_FEATURE_STATE_WINDOW" in GO
    fn = "func (s *State) RunWindow("
    assert fn in GO
    body = GO[GO.index(fn):]
    body = body[:body.index("\n}\n")]
    assert body.index("hasStateWindow()") < body.index("C.tad_run_state_window(")
    assert "C.tad_result_free(" in body


def test_window_kernels_are_hip_in_the_window_source():
    from theia_amd import build
    assert "tad_window.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_window.hip")).read()
    for name in ("k_win_bounds", "k_win_gather", "launch_win_bounds", "launch_win_gather", "win_hist_by_sort"):
        assert name in src, name
    assert "asm" not in src and "rocprim" not in src.lower()


def test_history_rule_is_the_documented_function_of_the_two_totals():
    """2 * (window points) <= (state points) sorts the window; anything above subtracts.  The library exports the very function
    tad_run_state_window decides with, so the boundary is pinned without a device."""
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    res, args = _capi.SYMBOLS["tad_window_history_by_sort"]
    assert res is ctypes.c_int and args == [ctypes.c_uint64, ctypes.c_uint64]
    assert re.search(r"int\s+tad_window_history_by_sort\s*\(\s*uint64_t window_points\s*,\s*uint64_t state_points\s*\)\s*;", CODE)
    for P, S, by_sort in ((0, 0, 1), (0, 10, 1), (1, 2, 1), (5, 10, 1), (6, 11, 0), (5, 9, 0), (10, 10, 0), (1 << 40, 1 << 41, 1),
                          ((1 << 40) + 1, 1 << 41, 0), (1, 1, 0)):
        assert lib.tad_window_history_by_sort(P, S) == by_sort, (P, S)
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_capi_view.cpp")).read()

    def body_of(head):
        body = src[src.index(head):]
        return body[:body.index("\n}\n")]
    assert "win_hist_by_sort(P, S)" in body_of("int view_call(")             # the one call path decides with the same function,
    for name in ("tad_run_state_window", "tad_run_state_keys"):               # both window calls go through it,
        assert "view_call(eng, st, job, \"%s\"" % name in body_of("int %s(" % name), name
    assert "return win_hist_by_sort(window_points, state_points)" in src      # and the exported function returns its result
