"""CPU tests of the boundary of the drop detector on states (include/tad.h: TAD_FEATURE_STATE_DROP, tad_drop_state, tad_drop_stream): the
feature bit, both prototypes and where the section stands in the header, the ctypes mirror and the unchanged struct sizes, the exported
symbols, tad_features() and the NULL-engine refusals without a device, the kernels' source, the Python wrappers against a library
without the bit, the Go binding's guard, and the periodical job beside the unchanged initial one.  No compute calls."""
import ctypes
import os
import re

import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_drop_state": ("int", ["tad_engine *e", "tad_state *s", "const tad_job *job", "int64_t from_t", "int64_t to_t", "uint64_t keep_points",
                               "tad_mem out_memory", "tad_result **out"]),
    "tad_drop_stream": ("int", ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_columns *cols", "tad_mem out_memory",
                                "tad_result **out"]),
}
GO_METHODS = {"tad_drop_state": "func (s *State) DropWindow(", "tad_drop_stream": "func (s *State) DropStream("}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_DROP\s+512u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_section_stands_between_the_key_retire_and_the_progress_calls():
    start = HEADER.index("TAD_FEATURE_STATE_DROP; check tad_features()")
    assert HEADER.index("int tad_keydict_compact(") < start < HEADER.index("int tad_drop_state(") < HEADER.index("int tad_drop_stream(") \
        < HEADER.index("int tad_progress(")
    section = " ".join(HEADER[start:HEADER.index("int tad_drop_state(")].replace("\n *", " ").split())     # the comment's text, unwrapped
    for must in ("periodical", "pairwise", "TAD_STATE_SERIES | TAD_STATE_TIMES", "bit for bit", "keys_no_result", "n >= drop_min_samples && n >= 2",
                 "TAD_ALGO_EWMA", "read-only", "each point once", "Lock order: the state, then a job context"):
        assert must in section, must
    # the old entry points still say that they refuse DROP, and name the new calls
    assert "tad_drop_stream" in HEADER[HEADER.index("streaming DBSCAN: a state WITH HISTORY"):HEADER.index("trimming a streaming state")]
    assert "tad_drop_state" in HEADER[HEADER.index("TAD_FEATURE_STATE_RUN; check tad_features()"):HEADER.index("int tad_run_state(")]


def test_ctypes_symbols_the_feature_constant_and_the_unchanged_structs(tmp_path):
    import subprocess
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_DROP == 512 and _capi.TAD_ABI_VERSION == 13
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args) and res is ctypes.c_int, name
    st = _capi.SYMBOLS["tad_drop_state"][1]
    assert st[3] == ctypes.c_int64 and st[4] == ctypes.c_int64 and st[5] == ctypes.c_uint64 and st[7] == ctypes.POINTER(ctypes.POINTER(_capi.Result))
    assert _capi.SYMBOLS["tad_drop_stream"][1] == _capi.SYMBOLS["tad_run_stream"][1]
    assert ctypes.sizeof(_capi.Job) == 136 and ctypes.sizeof(_capi.Columns) == 96                     # no existing struct grew
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "tad.h"\nint main(void) { printf("%zu %zu %u\\n", sizeof(tad_job), sizeof(tad_columns), '
                   'TAD_FEATURE_STATE_DROP); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["136", "96", "512"]


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 512 and f & _capi.TAD_FEATURE_STATE_DROP
    assert f & 1023 == 1023                                                                 # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    job = _capi.Job(algo=_capi.TAD_ALGO["DROP"])
    cols = _capi.Columns()
    res = ctypes.POINTER(_capi.Result)()
    assert lib.tad_drop_state(None, None, ctypes.byref(job), 0, 0, 0, _capi.TAD_MEM_HOST, ctypes.byref(res)) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_drop_stream(None, None, ctypes.byref(job), ctypes.byref(cols), _capi.TAD_MEM_HOST, ctypes.byref(res)) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert lib.tad_drop_state(None, None, None, 0, 0, 0, _capi.TAD_MEM_DEVICE, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert not res


def test_the_unit_is_hip_in_its_own_source():
    from theia_amd import build
    assert "tad_drop_state.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_drop_state.hip")).read()
    for name in ("k_ds_route", "k_ds_stats_lane", "k_ds_stats_wave", "k_ds_verdict", "k_ds_emit", "launch_ds_stats", "launch_ds_verdict", "launch_ds_emit",
                 "__shfl_xor", "__shared__", "__syncthreads", "code_anchor_drop_state"):
        assert name in src, name
    assert "asm" not in src and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert "fma(" not in src                                                                # d * d and the add stay two operations
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src) == ["stdint.h", "tad_internal.h"]
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    host = "".join(open(os.path.join(csrc, f)).read() for f in ("tad_capi.cpp", "tad_capi_view.cpp"))
    assert "int tad_drop_state(" in host and "int tad_drop_stream(" in host and "launch_ds_stats(" in host and "launch_win_route(" in host
    assert "code_anchor_drop_state()" in open(os.path.join(csrc, "tad_engine.cpp")).read()
    # the old entry points still refuse DROP
    assert "job->algo != TAD_ALGO_EWMA && job->algo != TAD_ALGO_DBSCAN && job->algo != TAD_ALGO_ARIMA" in host


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("a wrapper touched %s on a library without TAD_FEATURE_STATE_DROP" % name)


@pytest.mark.parametrize("lib", [_FakeLib(511), object()], ids=["without-the-bit", "without-tad_features"])
def test_the_wrappers_raise_cleanly_without_the_feature_bit(lib):
    import numpy as np
    from theia_amd import TadEngine, TadError, _capi
    eng = TadEngine.__new__(TadEngine)
    eng._lib, eng._h = lib, None
    with pytest.raises(TadError) as ei:
        eng.drop_state(object())
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_DROP" in ei.value.message
    with pytest.raises(TadError) as ei:
        eng.drop_stream(object(), np.zeros(1, np.uint64), np.zeros(1, np.int64), np.zeros(1, np.uint64))
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_DROP" in ei.value.message


def test_go_binding_binds_both_calls_behind_its_guard():
    assert "func hasStateDrop() bool" in GO and "C.tad_features()&C.TAD_FEATURE_STATE_DROP" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        assert body.index("hasStateDrop()") < body.index("C.%s(" % name), name
        assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", body), name      # no pointer into a Go slice crosses to the library
    assert "cj.algo = C.TAD_ALGO_DROP" in GO


def test_the_periodical_job_exists_and_the_initial_one_is_unchanged():
    from theia_amd import drop_detection as dd
    assert callable(dd.PeriodicalDropDetection) and hasattr(dd.PeriodicalDropDetection, "feed") and hasattr(dd.PeriodicalDropDetection, "window")
    with pytest.raises(AssertionError):
        next(dd.DropDetection().process("periodical", "id", "ep", "ingress", "2022-01-01", 5))
    assert "periodical" in dd.PeriodicalDropDetection.feed.__doc__
