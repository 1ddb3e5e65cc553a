"""CPU tests of the state trim's ABI (tad.h: TAD_FEATURE_STREAM_TRIM, TAD_STATE_TIMES and the four calls tad_state_trim,
tad_state_bytes, tad_state_export_times, tad_state_import_times): the header, the ctypes mirror, the library's exports and feature
query (which needs no device), the Python defaults and the Go binding's guard."""
import ctypes
import inspect
import os
import re
from job_helpers import HEADER, ROOT, header_define

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
NEW = ("tad_state_trim", "tad_state_bytes", "tad_state_export_times", "tad_state_import_times")


def test_header_defines_the_bits_and_declares_the_calls():
    assert header_define("TAD_STATE_TIMES") == "8u"      # (bit 4u stays unknown)
    assert header_define("TAD_FEATURE_STREAM_TRIM") == "8u"
    assert header_define("TAD_ABI_VERSION") == "13"     # additive: a flag, a feature bit and new functions, no ABI bump
    assert re.search(r"int tad_state_trim\(tad_engine \*e, tad_state \*s, uint64_t keep_points, int64_t keep_from_t, double ewma_alpha, "
                     r"uint64_t \*dropped\);", HEADER)
    assert re.search(r"int tad_state_bytes\(tad_engine \*e, const tad_state \*s, uint64_t \*bytes\);", HEADER)
    assert re.search(r"int tad_state_export_times\(tad_engine \*e, const tad_state \*s, int64_t \*t\);", HEADER)
    assert re.search(r"int tad_state_import_times\(tad_engine \*e, tad_state \*s, const int64_t \*t\);", HEADER)


def test_ctypes_binds_them_and_no_struct_grew():
    from theia_amd import _capi
    from theia_amd.engine import TadState
    assert (_capi.TAD_FEATURE_STREAM_TRIM, _capi.TAD_STATE_TIMES) == (8, 8)
    assert _capi.TAD_ABI_VERSION == 13
    restype, argtypes = _capi.SYMBOLS["tad_state_trim"]
    assert restype is ctypes.c_int and argtypes[2:5] == [ctypes.c_uint64, ctypes.c_int64, ctypes.c_double] and len(argtypes) == 6
    for name in NEW[1:]:
        restype, argtypes = _capi.SYMBOLS[name]
        assert restype is ctypes.c_int and len(argtypes) == 3, name
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136
    for m in ("trim", "nbytes", "export_times", "load_times"):
        assert callable(getattr(TadState, m)), m


def test_library_exports_them_and_reports_the_feature_without_a_device():
    from theia_amd import _capi
    lib = _capi.load_library()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    f = lib.tad_features()
    assert f & _capi.TAD_FEATURE_STREAM_TRIM and f & _capi.TAD_FEATURE_STREAM_ARIMA and f & _capi.TAD_FEATURE_STREAM_DBSCAN


def test_python_defaults():
    from theia_amd.engine import TadEngine, TadState
    assert inspect.signature(TadEngine.state_create).parameters["times"].default is False
    assert inspect.signature(TadState.__init__).parameters["times"].default is False
    p = inspect.signature(TadState.trim).parameters
    assert (p["keep_points"].default, p["keep_from"].default, p["alpha"].default) == (0, 0, 0.0)


def test_go_binding_asks_the_library_before_using_the_calls():
    for name in NEW:
        assert "C.%s(" % name in GO, name
    assert "C.tad_features()&C.TAD_FEATURE_STREAM_TRIM" in GO
    assert GO.index("func (e *Engine) NewStateWithSeries(") < GO.index("func (e *Engine) NewStateWithTimes(")
    body = GO[GO.index("func (e *Engine) NewStateWithTimes("):]
    body = body[:body.index("\n}\n")]
    assert body.index("hasStreamTrim()") < body.index("C.tad_state_create_ex(")
    assert "C.TAD_STATE_SERIES | C.TAD_STATE_TIMES" in body
    for fn in ("func (s *State) Trim(", "func (s *State) Bytes(", "func (s *State) ExportTimes(", "func (s *State) ImportTimes("):
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "hasStreamTrim()" in body, fn
