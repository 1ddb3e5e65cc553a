"""CPU tests of the change report's boundary (include/tad.h: TAD_FEATURE_STATE_ALERTS): the feature bit and the declarations in the header,
the ctypes mirror against the compiler's layout, the exported symbols, tad_features(), the refusals that need no device, and the Python
wrappers against a library without the bit.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from job_helpers import HEADER, ROOT

CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
MERGE_ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_columns *cols", "int64_t keep_from_t", "tad_merge_stats *stats",
              "tad_changes *ch"]
REPLACE_ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_columns *cols", "uint32_t flags", "int64_t from_t", "int64_t to_t",
                "int64_t keep_from_t", "tad_replace_stats *stats", "tad_changes *ch"]
CHANGES_FIELDS = ["key_since", "len", "memory", "keys_changed", "points_changed", "min_t", "max_t"]


def _proto(name):
    m = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert m and m.group(1) == "int", name
    return [" ".join(a.split()) for a in m.group(2).split(",")]


def test_header_defines_the_bit_the_struct_and_the_calls_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_ALERTS\s+131072u\b", HEADER)
    assert re.search(r"#define\s+TAD_NO_CHANGE\s+INT64_MAX\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    assert _proto("tad_state_merge_changes") == MERGE_ARGS
    assert _proto("tad_state_replace_changes") == REPLACE_ARGS
    # the existing calls keep their signatures: the new ones with the report dropped
    assert _proto("tad_state_merge") == MERGE_ARGS[:-1] and _proto("tad_state_replace") == REPLACE_ARGS[:-1]
    body = re.search(r"typedef struct \{([^}]*)\} tad_changes;", CODE, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body.replace("min_t, max_t", "min_t; int64_t max_t")) == CHANGES_FIELDS
    section = HEADER[HEADER.index("TAD_FEATURE_STATE_ALERTS; check tad_features()"):HEADER.index("int tad_state_merge_changes(")]
    for must in ("in exactly one of W and W'", "in both with different values", "a sum merge of value 0", "a max merge of a value not", "a replace by the held value",
                 "keys_changed == 0 the second time", "keys_changed <= stats.keys_touched", "every entry TAD_NO_CHANGE", "NULL\n * with len == 0",
                 "copied out only on success", "content is unspecified", "NULL report"):
        assert must in section, must


def test_ctypes_mirror_matches_the_compilers_layout(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_ALERTS == 131072 and _capi.TAD_NO_CHANGE == 2**63 - 1 and _capi.TAD_ABI_VERSION == 13
    for name, args, stats in (("tad_state_merge_changes", MERGE_ARGS, _capi.MergeStats), ("tad_state_replace_changes", REPLACE_ARGS, _capi.ReplaceStats)):
        res, argtypes = _capi.SYMBOLS[name]
        assert res is ctypes.c_int and len(argtypes) == len(args)
        assert argtypes[:-1] == _capi.SYMBOLS[name[:-len("_changes")]][1]
        assert argtypes[-2] == ctypes.POINTER(stats) and argtypes[-1] == ctypes.POINTER(_capi.Changes)
    S = _capi.Changes
    assert [n for n, _ in S._fields_] == CHANGES_FIELDS
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.MergeStats, _capi.ReplaceStats, _capi.CompactStats)] == [136, 96, 104, 120, 96]
    probe = ["sizeof(tad_changes)"] + ["offsetof(tad_changes, %s)" % f for f in CHANGES_FIELDS]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("' + "%zu " * len(probe) + '%lld\\n", ' + ", ".join(probe) +
                   ", (long long)TAD_NO_CHANGE); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in CHANGES_FIELDS] + [_capi.TAD_NO_CHANGE]
    assert ctypes.sizeof(S) == 56


def test_library_exports_the_symbols_and_refuses_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_state_merge_changes") and hasattr(lib, "tad_state_replace_changes")
    f = lib.tad_features()
    assert f & 131072 and f & 131071 == 131071           # the new bit, and every earlier one
    assert lib.tad_abi_version() == 13
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    job, cols = _capi.Job(), _capi.Columns()
    arr = np.full(4, 7, np.int64)
    for with_report in (True, False):
        ch = _capi.Changes(key_since=arr.ctypes.data, len=4, memory=0, keys_changed=3, points_changed=3, min_t=3, max_t=3)
        rep = ctypes.byref(ch) if with_report else None
        ms, rs = _capi.MergeStats(), _capi.ReplaceStats()
        ctypes.memset(ctypes.byref(ms), 0x5A, ctypes.sizeof(ms))
        ctypes.memset(ctypes.byref(rs), 0x5A, ctypes.sizeof(rs))
        # a NULL engine, a NULL state: refused before anything is touched, the stats zeroed as the calls without a report zero them
        assert lib.tad_state_merge_changes(None, None, ctypes.byref(job), ctypes.byref(cols), 0, ctypes.byref(ms), rep) == inv
        assert lib.tad_state_replace_changes(None, None, ctypes.byref(job), ctypes.byref(cols), 0, 0, 0, 0, ctypes.byref(rs), rep) == inv
        assert bytes(ms) == bytes(ctypes.sizeof(ms)) and bytes(rs) == bytes(ctypes.sizeof(rs))
        assert lib.tad_state_replace_changes(None, None, None, None, _capi.TAD_REPLACE_RANGE, 5, 3, 0, None, rep) == inv
    assert (arr == 7).all()


SINCE_ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_report_window *w", "tad_mem out_memory", "tad_result **out"]
WINDOW_FIELDS = ["from_t", "to_t", "keep_points", "key_keep", "key_since", "since_t", "num_keys", "key_memory"]


def test_the_since_calls_in_the_header_the_mirror_and_the_library(tmp_path):
    from theia_amd import _capi, build
    assert _proto("tad_run_state_since") == SINCE_ARGS and _proto("tad_drop_state_since") == SINCE_ARGS
    body = re.search(r"typedef struct \{([^}]*)\} tad_report_window;", CODE, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body.replace("from_t, to_t", "from_t; int64_t to_t")) == WINDOW_FIELDS
    start = HEADER.index("Judge the window, report from a time on")
    section = HEADER[start:HEADER.index("int tad_run_state_since(")]
    for must in ("REPORTED iff", "counts as NOT SELECTED", "restricted to the reported points", "bit for bit", "WHOLE window",
                 "IS the *_keys call", "Read-only", "arima_fits counts the fits actually run", "host_syncs", "not reported"):
        assert must in section, must
    S = _capi.ReportWindow
    assert [n for n, _ in S._fields_] == WINDOW_FIELDS
    for name in ("tad_run_state_since", "tad_drop_state_since"):
        res, argtypes = _capi.SYMBOLS[name]
        assert res is ctypes.c_int and len(argtypes) == len(SINCE_ARGS) and argtypes[3] == ctypes.POINTER(S)
    probe = ["sizeof(tad_report_window)"] + ["offsetof(tad_report_window, %s)" % f for f in WINDOW_FIELDS]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("' + "%zu " * len(probe) + '\\n", ' + ", ".join(probe) +
                   "); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in WINDOW_FIELDS] and ctypes.sizeof(S) == 64
    build.build_library()
    lib = _capi.load_library()
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    w, job = S(since_t=5), _capi.Job()
    res = ctypes.POINTER(_capi.Result)()
    for fn in (lib.tad_run_state_since, lib.tad_drop_state_since):
        assert fn(None, None, ctypes.byref(job), ctypes.byref(w), 0, ctypes.byref(res)) == inv and not res


def test_the_python_wrappers_of_the_since_calls():
    import inspect
    from theia_amd import TadError, _capi
    from theia_amd.engine import TadEngine
    from theia_amd.stream_detection import StreamingAnomalyDetection
    from theia_amd.drop_detection import PeriodicalDropDetection
    p = list(inspect.signature(TadEngine.run_state_since).parameters)
    assert p[:8] == ["self", "state", "since_t", "key_since", "key_keep", "from_t", "to_t", "keep_points"] and "algo" in p
    assert list(inspect.signature(TadEngine.drop_state_since).parameters)[:8] == p[:8]
    assert list(inspect.signature(StreamingAnomalyDetection.feed_alerts).parameters)[:5] == ["self", "flows", "algo_type", "tad_id", "replace"]
    assert list(inspect.signature(StreamingAnomalyDetection.poll_alerts).parameters)[:6] == ["self", "client", "now", "lag_s", "algo_type", "tad_id"]
    assert inspect.signature(PeriodicalDropDetection.feed).parameters["partial"].default is False
    assert inspect.signature(PeriodicalDropDetection.feed_flows).parameters["partial"].default is False
    eng = object.__new__(TadEngine)
    eng._lib = _OldLib()
    for call in (eng.run_state_since, eng.drop_state_since):
        with pytest.raises(TadError) as ei:
            call(_State(), since_t=5)
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_ALERTS" in str(ei.value)


class _OldLib:
    """a library of before the feature: every earlier bit"""

    def tad_features(self):
        return 131071

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STATE_ALERTS" % name)


class _State:
    num_keys = 3


def test_the_wrappers_refuse_a_report_from_a_library_without_the_bit():
    from theia_amd import TadError, _capi
    from theia_amd.engine import TadEngine
    eng = object.__new__(TadEngine)
    eng._lib = _OldLib()
    for mode in ("host", "device", "counters"):
        with pytest.raises(TadError) as ei:
            eng._changes(_State(), mode)
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_ALERTS" in str(ei.value)
    assert eng._changes(_State(), None) == (None, None)
    with pytest.raises(TadError):
        eng._changes(_State(), "somewhere")
