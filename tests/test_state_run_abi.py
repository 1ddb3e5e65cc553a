"""CPU tests of tad_run_state's ABI (tad.h: TAD_FEATURE_STATE_RUN and the call): the header, the ctypes mirror, the library's export
and feature query (which needs no device), the Python defaults and the Go binding's guard."""
import ctypes
import inspect
import os
import re
from job_helpers import HEADER, ROOT, header_define

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()


def test_header_defines_the_bit_and_declares_the_call():
    assert header_define("TAD_FEATURE_STATE_RUN") == "16u"
    assert header_define("TAD_ABI_VERSION") == "13"     # additive: a feature bit and a function, no ABI bump
    assert re.search(r"int tad_run_state\(tad_engine \*e, tad_state \*s, const tad_job \*job, tad_mem out_memory, tad_result \*\*out\);", HEADER)
    # documented as its own section, after the trim section
    assert HEADER.index("int tad_state_import_times(") < HEADER.index("TAD_FEATURE_STATE_RUN; check tad_features()") < HEADER.index("int tad_run_state(")


def test_ctypes_binds_it_and_no_struct_grew():
    from theia_amd import _capi
    from theia_amd.engine import TadEngine
    assert _capi.TAD_FEATURE_STATE_RUN == 16
    assert _capi.TAD_ABI_VERSION == 13
    restype, argtypes = _capi.SYMBOLS["tad_run_state"]
    assert restype is ctypes.c_int and len(argtypes) == 5
    assert argtypes[2] == ctypes.POINTER(_capi.Job) and argtypes[3] is ctypes.c_int and argtypes[4] == ctypes.POINTER(ctypes.POINTER(_capi.Result))
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136
    assert callable(TadEngine.run_state)


def test_library_exports_it_and_reports_the_feature_without_a_device():
    from theia_amd import _capi
    lib = _capi.load_library()
    fn = lib.tad_run_state
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    f = lib.tad_features()
    assert f & 16 and f & _capi.TAD_FEATURE_STATE_RUN
    assert f & _capi.TAD_FEATURE_STREAM_TRIM and f & _capi.TAD_FEATURE_STREAM_ARIMA and f & _capi.TAD_FEATURE_STREAM_DBSCAN   # (the earlier bits stay)


def test_python_defaults():
    from theia_amd.engine import TadEngine
    p = inspect.signature(TadEngine.run_state).parameters
    assert list(p)[:2] == ["self", "state"]
    assert (p["algo"].default, p["alpha"].default, p["eps"].default, p["min_samples"].default, p["maxiter"].default) == ("EWMA", 0.0, 0.0, 0, 0)
    assert (p["emit_all"].default, p["out"].default, p["job_id"].default) == (False, "host", "")


def test_go_binding_asks_the_library_before_using_the_call():
    assert "C.tad_run_state(" in GO
    assert "C.tad_features()&C.TAD_FEATURE_STATE_RUN" in GO
    fn = "func (s *State) Run("
    assert fn in GO
    body = GO[GO.index(fn):]
    body = body[:body.index("\n}\n")]
    assert body.index("hasStateRun()") < body.index("C.tad_run_state(")
    assert "C.tad_result_free(" in body
