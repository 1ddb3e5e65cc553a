"""CPU tests of the boundary of retiring dead keys (include/tad.h: TAD_FEATURE_KEY_RETIRE, tad_state_compact, tad_keydict_compact): the
feature bit, the prototypes and the stats struct in the header, where the section stands, the ctypes mirror, the exported symbols,
tad_features() and the NULL-engine refusals without a device, the kernels' source, the Python wrappers against a library without the bit,
and the Go binding's guard.  No compute calls."""
import ctypes
import os
import re
import subprocess

import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_state_compact": ("int", ["tad_engine *e", "tad_state *s", "int64_t retire_before_t", "uint64_t *remap", "tad_mem remap_memory",
                                  "tad_compact_stats *stats"]),
    "tad_keydict_compact": ("int", ["tad_engine *e", "tad_keydict *d", "const uint64_t *remap", "uint64_t remap_len", "tad_mem remap_memory",
                                    "uint64_t *num_keys"]),
}
STATS_FIELDS = [("uint64_t", "keys_before"), ("uint64_t", "keys_after"), ("uint64_t", "num_keys"), ("uint64_t", "keys_unseen"), ("uint64_t", "keys_idle"),
                ("uint64_t", "points_dropped"), ("uint64_t", "series_points_moved"), ("uint64_t", "history_points_moved"), ("uint64_t", "bytes_before"),
                ("uint64_t", "bytes_after"), ("int32_t", "job_context"), ("int32_t", "reserved"), ("float", "ms_total"), ("float", "reserved1")]
GO_METHODS = {"tad_state_compact": "func (s *State) Compact(", "tad_keydict_compact": "func (d *KeyDict) Compact("}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_KEY_RETIRE\s+256u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_declares_the_stats_struct_field_for_field():
    body = re.search(r"typedef struct \{([^}]*)\}\s*tad_compact_stats;", CODE, flags=re.S)
    assert body, "tad_compact_stats is not declared"
    fields = []
    for decl in body.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            typ, names = decl.split(" ", 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    assert fields == STATS_FIELDS


def test_header_documents_the_contract_between_the_dictionary_and_the_progress_calls():
    start = HEADER.index("TAD_FEATURE_KEY_RETIRE; check tad_features()")
    assert HEADER.index("int tad_keydict_import(") < start < HEADER.index("int tad_state_compact(") < HEADER.index("int tad_keydict_compact(") \
        < HEADER.index("int tad_progress(")
    section = HEADER[start:HEADER.index("int tad_state_compact(")]
    for must in ("retire_before_t", "TAD_KEY_SKIP", "max(m, 1)", "first appearance", "bit for bit", "workspace_limit", "TAD_ERR_GRID_TOO_LARGE", "stale",
                 "identity", "points_dropped == 0", "remap_len", "0, 1, ..., m - 1", "tad_keydict_import", "tad_keydict_bytes",
                 "Lock order: the state, then a job context", "Lock order: the dictionary, then a job context"):
        assert must in section, must
    # the dictionary's own section names the one exception to "ids never move"
    kd = HEADER[HEADER.index("TAD_FEATURE_KEY_DICT; check tad_features()"):HEADER.index("int tad_keydict_create(")]
    assert "never" in kd and "tad_keydict_compact" in kd


def test_ctypes_symbols_the_feature_constant_and_the_struct_against_gcc(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_KEY_RETIRE == 256 and _capi.TAD_ABI_VERSION == 13
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args) and res is ctypes.c_int, name
    assert _capi.SYMBOLS["tad_state_compact"][1][2] == ctypes.c_int64 and _capi.SYMBOLS["tad_state_compact"][1][5] == ctypes.POINTER(_capi.CompactStats)
    assert _capi.SYMBOLS["tad_keydict_compact"][1][3] == ctypes.c_uint64
    assert [n for n, _ in _capi.CompactStats._fields_] == [n for _, n in STATS_FIELDS]
    assert ctypes.sizeof(_capi.CompactStats) == 96
    assert ctypes.sizeof(_capi.KeyColumns) == 56 and ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.MergeStats) == 104   # no existing struct grew
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(tad_compact_stats), '
                   'offsetof(tad_compact_stats, job_context), offsetof(tad_compact_stats, ms_total)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_capi.CompactStats), _capi.CompactStats.job_context.offset, _capi.CompactStats.ms_total.offset]


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 256 and f & _capi.TAD_FEATURE_KEY_RETIRE
    assert f & 511 == 511                                                                   # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    remap = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    cs = _capi.CompactStats(keys_before=5, num_keys=5)
    assert lib.tad_state_compact(None, None, 0, remap, _capi.TAD_MEM_HOST, ctypes.byref(cs)) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert list(remap) == [7, 7, 7, 7] and cs.keys_before == 5 and cs.num_keys == 5
    n = ctypes.c_uint64(5)
    assert lib.tad_keydict_compact(None, None, remap, 4, _capi.TAD_MEM_HOST, ctypes.byref(n)) == _capi.TAD_ERR_INVALID_ARGUMENT and n.value == 5
    assert lib.tad_keydict_compact(None, None, None, 0, _capi.TAD_MEM_DEVICE, None) == _capi.TAD_ERR_INVALID_ARGUMENT


def test_the_unit_is_hip_in_its_own_source():
    from theia_amd import build
    assert "tad_compact.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "theia_amd", "csrc", "tad_compact.hip")).read()
    for name in ("k_compact_mark", "k_compact_keys", "k_compact_copy", "k_kd_compact", "launch_compact_mark", "launch_compact_keys", "launch_compact_copy",
                 "launch_kd_compact", "chunk_key(", "kHistChunk", "__ballot", "code_anchor_compact"):
        assert name in src, name
    assert "asm" not in src and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src) == ["tad_internal.h"]
    host = "".join(open(os.path.join(ROOT, "theia_amd", "csrc", f)).read() for f in ("tad_capi.cpp", "tad_capi_view.cpp", "tad_capi_state.cpp", "tad_capi_keydict.cpp"))
    assert "int tad_state_compact(" in host and "int tad_keydict_compact(" in host and "launch_scan(" in host and "launch_kd_rehash(" in host


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("a wrapper touched %s on a library without TAD_FEATURE_KEY_RETIRE" % name)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        raise AssertionError("no call may be made")


@pytest.mark.parametrize("lib", [_FakeLib(255), object()], ids=["without-the-bit", "without-tad_features"])
def test_the_wrappers_raise_cleanly_without_the_feature_bit(lib):
    from theia_amd import KeyDict, TadError, _capi
    from theia_amd.engine import TadState
    st = TadState.__new__(TadState)
    st._engine, st._h, st.num_keys = _FakeEngine(lib), None, 4
    with pytest.raises(TadError) as ei:
        st.compact()
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_KEY_RETIRE" in ei.value.message and st.num_keys == 4
    d = KeyDict.__new__(KeyDict)
    d._engine, d._h, d.n_cols = _FakeEngine(lib), None, 2
    with pytest.raises(TadError) as ei:
        d.compact([0, 1])
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_KEY_RETIRE" in ei.value.message


def test_go_binding_binds_both_calls_behind_its_guard():
    assert "func hasKeyRetire() bool" in GO and "C.tad_features()&C.TAD_FEATURE_KEY_RETIRE" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        assert body.index("hasKeyRetire()") < body.index("C.%s(" % name), name
        # the remap crosses in C memory: no pointer into a Go slice is handed to the library
        assert ("C.calloc(" in body or "cColumn(" in body) and "C.free(" in body, name
        assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", body), name
