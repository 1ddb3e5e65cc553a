"""CPU tests of tad_state_merge's boundary (include/tad.h): the feature bit and the prototype in the header, the ctypes mirror against the
compiler's layout, the exported symbol, tad_features() without a device, the Python method's signature and the Go binding's guard.  No
compute calls."""
import ctypes
import inspect
import os
import re
import subprocess
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_MERGE\s+32u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


def test_header_declares_the_call_after_tad_run_state():
    proto = re.search(r"int\s+tad_state_merge\s*\(([^;]*?)\)\s*;", CODE, flags=re.S)
    assert proto, "tad_state_merge is not declared"
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    assert args == ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_columns *cols", "int64_t keep_from_t", "tad_merge_stats *stats"]
    assert CODE.index("int tad_run_state(") < CODE.index("tad_merge_stats;") < CODE.index("int tad_state_merge(") < CODE.index("int tad_progress(")


def test_merge_stats_fields_are_one_declarator_per_line():
    body = re.search(r"typedef struct \{([^{}]*)\} tad_merge_stats;", CODE).group(1)
    fields = re.findall(r"\b(\w+)\s*;", body)
    from theia_amd import _capi
    assert fields == [f[0] for f in _capi.MergeStats._fields_]
    assert "," not in body


def test_ctypes_mirror_matches_the_c_compiler(tmp_path):
    from theia_amd import _capi
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",sizeof(tad_merge_stats),'
                    'sizeof(tad_columns),sizeof(tad_job),offsetof(tad_merge_stats,keys_replayed),offsetof(tad_merge_stats,stage0_path),'
                    'offsetof(tad_merge_stats,ms_total));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    ms = _capi.MergeStats
    assert sizes == [ctypes.sizeof(ms), ctypes.sizeof(_capi.Columns), ctypes.sizeof(_capi.Job), ms.keys_replayed.offset, ms.stage0_path.offset,
                     ms.ms_total.offset]
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136      # no existing struct grew
    assert ctypes.sizeof(ms) == 104


def test_ctypes_symbol_entry():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_MERGE == 32 and _capi.TAD_ABI_VERSION == 13
    res, args = _capi.SYMBOLS["tad_state_merge"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_capi.Job), ctypes.POINTER(_capi.Columns), ctypes.c_int64,
                    ctypes.POINTER(_capi.MergeStats)]


def test_library_exports_the_symbol_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_state_merge")
    f = lib.tad_features()
    assert f & 32
    assert f & (1 | 2 | 4 | 8 | 16) == 31
    assert lib.tad_abi_version() == 13


def test_python_method_signature():
    from theia_amd.engine import TadEngine
    sig = inspect.signature(TadEngine.merge_stream)
    got = [(p.name, p.default) for p in sig.parameters.values()]
    E = inspect.Parameter.empty
    assert got == [("self", E), ("state", E), ("key_id", E), ("flow_end_s", E), ("value", E), ("agg_flow", ""), ("value_op", "auto"), ("lattice", None),
                   ("alpha", 0.0), ("keep_from", 0), ("job_id", ""), ("num_keys", None), ("key_id2", None)]
    run = inspect.signature(TadEngine.run_stream).parameters
    for name, default in got[1:]:
        if name in run:
            assert run[name].default == default, name       # shared parameters keep run_stream's defaults


def test_go_binding_guards_the_call():
    assert "func hasStateMerge() bool" in GO and "C.TAD_FEATURE_STATE_MERGE" in GO
    m = re.search(r"func \(s \*State\) Merge\(job Job, cols Columns, keepFrom int64\) \(MergeStats, error\) \{(.*?)\n\}\n", GO, flags=re.S)
    assert m, "State.Merge is missing"
    body = m.group(1)
    assert "hasStateMerge()" in body and "C.tad_state_merge(" in body
    assert body.index("hasStateMerge()") < body.index("C.tad_state_merge(")


def test_merge_kernels_are_part_of_the_build():
    from theia_amd import build
    assert "tad_merge.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_merge.hip")).read()
    assert "asm" not in src and "rocprim" not in src.lower()
    # every kernel of the merge and of the replace is this unit's: one series kernel, the sum and the maximum among its rules
    for name in ("k_merge_classify", "k_merge_range", "k_merge_keys", "k_merge_series", "k_merge_moments", "launch_series_as<MERGE_SUM, false>",
                 "launch_series_as<MERGE_MAX, false>"):
        assert name in src, name
    assert not os.path.exists(os.path.join(ROOT, "theia_amd", "csrc", "tad_replace.hip"))
