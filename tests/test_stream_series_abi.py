"""CPU tests of the streaming ARIMA detector's ABI (tad.h: TAD_FEATURE_STREAM_ARIMA, TAD_STATE_SERIES and the three series calls):
the header, the ctypes mirror, the library's exports and feature query (which needs no device), the Python defaults and the Go
binding's guard."""
import ctypes
import inspect
import os
import re
from job_helpers import HEADER, ROOT, header_define

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
NEW = ("tad_state_series_points", "tad_state_export_series", "tad_state_import_series")


def test_header_defines_the_bits_and_declares_the_calls():
    assert header_define("TAD_STATE_SERIES") == "2u"
    assert header_define("TAD_FEATURE_STREAM_ARIMA") == "4u"
    assert header_define("TAD_ABI_VERSION") == "13"     # additive: a flag, a feature bit and new functions, no ABI bump
    assert re.search(r"int tad_state_series_points\(tad_engine \*e, const tad_state \*s, uint64_t \*n_points\);", HEADER)
    assert re.search(r"int tad_state_export_series\(tad_engine \*e, const tad_state \*s, uint64_t \*len, uint64_t \*values\);", HEADER)
    assert re.search(r"int tad_state_import_series\(tad_engine \*e, tad_state \*s, const uint64_t \*len, const uint64_t \*values\);", HEADER)


def test_ctypes_binds_them_and_no_struct_grew():
    from theia_amd import _capi
    from theia_amd.engine import TadState
    assert (_capi.TAD_FEATURE_STREAM_ARIMA, _capi.TAD_STATE_SERIES) == (4, 2)
    assert _capi.TAD_ABI_VERSION == 13
    for name in NEW:
        restype, argtypes = _capi.SYMBOLS[name]
        assert restype is ctypes.c_int and len(argtypes) in (3, 4), name
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136
    for m in ("series_points", "export_series", "load_series"):
        assert callable(getattr(TadState, m)), m


def test_library_exports_them_and_reports_the_feature_without_a_device():
    from theia_amd import _capi
    lib = _capi.load_library()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    f = lib.tad_features()
    assert f & _capi.TAD_FEATURE_STREAM_ARIMA and f & _capi.TAD_FEATURE_STREAM_DBSCAN and f & _capi.TAD_FEATURE_NARROW_COLUMNS


def test_python_defaults():
    from theia_amd.engine import TadEngine, TadState
    assert inspect.signature(TadEngine.state_create).parameters["series"].default is False
    assert inspect.signature(TadEngine.state_create).parameters["history"].default is False
    assert inspect.signature(TadState.__init__).parameters["series"].default is False
    assert inspect.signature(TadEngine.run_stream).parameters["maxiter"].default == 0


def test_go_binding_asks_the_library_before_creating_a_series_state():
    for name in NEW:
        assert "C.%s(" % name in GO, name
    assert "C.TAD_FEATURE_STREAM_ARIMA" in GO
    assert GO.index("func (e *Engine) NewStateWithHistory(") < GO.index("func (e *Engine) NewStateWithSeries(")
    body = GO[GO.index("func (e *Engine) NewStateWithSeries("):]
    body = body[:body.index("\n}\n")]
    assert "C.tad_features()&C.TAD_FEATURE_STREAM_ARIMA" in GO
    assert body.index("hasStreamARIMA()") < body.index("C.tad_state_create_ex(")
    assert "C.TAD_STATE_SERIES" in body
    for fn in ("func (s *State) SeriesPoints(", "func (s *State) ExportSeries(", "func (s *State) ImportSeries("):
        assert fn in GO, fn
    assert GO.count("cj.arima_maxiter = C.int32_t(job.ARIMAMaxIter)") == 2
