"""CPU tests of the streaming DBSCAN detector's ABI (tad.h: TAD_FEATURE_STREAM_DBSCAN, TAD_STATE_HISTORY and the four history calls):
the header, the ctypes mirror, the library's exports and feature query (which needs no device) and the Go binding's guard."""
import ctypes
import os
import re
from job_helpers import HEADER, ROOT, header_define

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
NEW = ("tad_state_create_ex", "tad_state_history_points", "tad_state_export_history", "tad_state_import_history")


def test_header_defines_the_bits_and_declares_the_calls():
    assert header_define("TAD_FEATURE_STREAM_DBSCAN") == "2u"
    assert header_define("TAD_STATE_HISTORY") == "1u"
    assert header_define("TAD_ABI_VERSION") == "13"     # additive: a feature bit and new functions, no ABI bump
    assert re.search(r"int tad_state_create_ex\(tad_engine \*e, uint64_t num_keys, uint32_t flags, tad_state \*\*out\);", HEADER)
    assert re.search(r"int tad_state_history_points\(tad_engine \*e, const tad_state \*s, uint64_t \*n_points\);", HEADER)
    assert re.search(r"int tad_state_export_history\(tad_engine \*e, const tad_state \*s, uint64_t \*len, uint64_t \*values\);", HEADER)
    assert re.search(r"int tad_state_import_history\(tad_engine \*e, tad_state \*s, const uint64_t \*len, const uint64_t \*values\);", HEADER)


def test_ctypes_binds_them_and_no_struct_grew():
    from theia_amd import _capi
    from theia_amd.engine import TadState
    assert (_capi.TAD_FEATURE_STREAM_DBSCAN, _capi.TAD_STATE_HISTORY) == (2, 1)
    assert _capi.TAD_ABI_VERSION == 13
    for name in NEW:
        restype, argtypes = _capi.SYMBOLS[name]
        assert restype is ctypes.c_int, name
    assert _capi.SYMBOLS["tad_state_create_ex"][1][2] is ctypes.c_uint32
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136
    for m in ("history_points", "export_history", "load_history"):
        assert callable(getattr(TadState, m)), m


def test_library_exports_them_and_reports_both_features_without_a_device():
    from theia_amd import _capi
    lib = _capi.load_library()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    f = lib.tad_features()
    assert f & _capi.TAD_FEATURE_NARROW_COLUMNS and f & _capi.TAD_FEATURE_STREAM_DBSCAN


def test_run_stream_takes_the_detector_and_its_parameters():
    import inspect
    from theia_amd.engine import TadEngine
    sig = inspect.signature(TadEngine.run_stream).parameters
    assert sig["algo"].default == "EWMA" and sig["eps"].default == 0.0 and sig["min_samples"].default == 0
    assert inspect.signature(TadEngine.state_create).parameters["history"].default is False


def test_go_binding_asks_the_library_before_creating_a_history_state():
    for name in NEW:
        assert "C.%s(" % name in GO, name
    assert "C.TAD_FEATURE_STREAM_DBSCAN" in GO
    guard = GO.index("C.tad_features()&C.TAD_FEATURE_STREAM_DBSCAN")
    assert guard < GO.index("C.tad_state_create_ex(")
    body = GO[GO.index("func (e *Engine) NewStateWithHistory("):]
    body = body[:body.index("\n}\n")]
    assert body.index("hasStreamDBSCAN()") < body.index("C.tad_state_create_ex(")
    for fn in ("func (s *State) HistoryPoints(", "func (s *State) ExportHistory(", "func (s *State) ImportHistory("):
        assert fn in GO, fn
    assert "cj.dbscan_eps = C.double(job.DBSCANEps)" in GO
