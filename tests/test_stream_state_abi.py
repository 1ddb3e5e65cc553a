"""CPU: the ABI-13 state calls of the streaming EWMA detector (tad_state_resize, tad_state_import) are declared by include/tad.h,
bound with argtypes by theia_amd/_capi.py and called by the Go binding."""
import ctypes as C
import os
import re

from theia_amd import _capi
from theia_amd.engine import TadState
from job_helpers import ROOT

NEW = ("tad_state_resize", "tad_state_import")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_calls_at_abi_13():
    h = _read("include", "tad.h")
    assert re.search(r"#define TAD_ABI_VERSION 13\b", h)
    assert re.search(r"int tad_state_resize\(tad_engine \*e, tad_state \*s, uint64_t new_num_keys\);", h)
    assert re.search(r"int tad_state_import\(tad_engine \*e, tad_state \*s, const uint32_t \*n, const double \*avg, const double \*m2, "
                     r"const double \*ewma,\s+const int64_t \*last_t\);", h)
    assert _capi.TAD_ABI_VERSION == 13


def test_ctypes_binds_them_with_argtypes():
    restype, argtypes = _capi.SYMBOLS["tad_state_resize"]
    assert restype is C.c_int and len(argtypes) == 3 and argtypes[2] is C.c_uint64
    restype, argtypes = _capi.SYMBOLS["tad_state_import"]
    assert restype is C.c_int and len(argtypes) == 7
    assert callable(TadState.resize) and callable(TadState.load)


def test_library_exports_them():
    from theia_amd import build
    assert "tad_capi_state.cpp" in build.SOURCES     # the unit that implements them
    lib = _capi.load_library()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int


def test_go_binding_calls_them():
    go = _read("go", "tadengine", "tadengine.go")
    for name in NEW:
        assert "C.%s(" % name in go
    assert "func (s *State) Resize(" in go and "func (s *State) Import(" in go
