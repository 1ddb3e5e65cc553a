"""CPU tests of the boundary of the drop job's flow-row query (include/tad.h: TAD_FEATURE_DROP_ROWS, tad_drop_select, tad_drop_rows_free):
the feature bit, the exact prototypes and where the section stands in the header, the ctypes mirror and the unchanged struct sizes, the
exported symbols, tad_features() and the NULL-engine refusal without a device, the kernels' source, the Python wrapper against a library
without the bit, the Go binding's guard — and the two host forms of the query in tests/drop_query_ref.py held against each other: the
query's two GROUP BYs compose to the sum of count = 1 per (tuple, day) of the selected rows.  No compute calls."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import drop_query_ref as dq  # noqa: E402
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_drop_select": ("int", ["tad_engine *e", "const tad_drop_flow_columns *cols", "int64_t start_time", "int64_t end_time", "tad_mem out_memory",
                                "tad_drop_rows **out"]),
    "tad_drop_rows_free": ("void", ["tad_engine *e", "tad_drop_rows *r"]),
}
FLOW_FIELDS = ["n_rows", "ingress_action", "egress_action", "flow_start_s", "flow_end_s", "src_ip", "src_pod_ns", "src_pod_name", "dst_ip", "dst_pod_ns",
               "dst_pod_name", "src_pod_null", "dst_pod_null", "keep", "flags", "memory"]
ROWS_FIELDS = ["n_rows", "endpoint_kind", "endpoint_ns", "endpoint_name", "direction", "day_s", "count", "row", "memory"]


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_DROP_ROWS\s+1024u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_every_call_with_its_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def struct_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, CODE).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            out += [re.sub(r"[\s*]", " ", first).split()[-1]] + [m.strip(" *") for m in more]
    return out


def test_header_section_stands_between_the_state_drop_and_the_progress_calls():
    start = HEADER.index("TAD_FEATURE_DROP_ROWS; check tad_features()")
    assert HEADER.index("int tad_drop_stream(") < start < HEADER.index("int tad_drop_select(") < HEADER.index("void tad_drop_rows_free(") \
        < HEADER.index("int tad_progress(")
    assert struct_fields("tad_drop_flow_columns") == FLOW_FIELDS and struct_fields("tad_drop_rows") == ROWS_FIELDS
    section = " ".join(HEADER[start:HEADER.index("#define TAD_FEATURE_DROP_ROWS")].replace("\n *", " ").split())     # the comment's text, unwrapped
    for must in ("dropDetection.go:36-190", "ingress wins when both actions drop", "Ingress rows describe the destination", "INPUT ORDER",
                 "floor, not truncation", "count = 1", "contains '/'", "Kubernetes forbids", "two GROUP BYs composed", "merges again",
                 "TAD_FLAG_TIME_U32", "zero-extended", "reads its inputs only", "end_time != 0 with flow_end_s == NULL", "tad_drop_rows_free"):
        assert must in section, must


def test_ctypes_mirror_the_feature_constant_and_the_unchanged_structs(tmp_path):
    import subprocess
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_DROP_ROWS == 1024 and _capi.TAD_ABI_VERSION == 13
    assert [f[0] for f in _capi.DropFlowColumns._fields_] == FLOW_FIELDS and [f[0] for f in _capi.DropRows._fields_] == ROWS_FIELDS
    sel = _capi.SYMBOLS["tad_drop_select"]
    assert sel[0] is ctypes.c_int and sel[1] == [ctypes.c_void_p, ctypes.POINTER(_capi.DropFlowColumns), ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.POINTER(_capi.DropRows))]
    assert _capi.SYMBOLS["tad_drop_rows_free"] == (None, [ctypes.c_void_p, ctypes.POINTER(_capi.DropRows)])
    sizes = [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.Points, _capi.KeyColumns, _capi.DropFlowColumns, _capi.DropRows)]
    assert sizes[:2] == [136, 96]                                                          # no existing struct grew
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %u %zu %zu %zu\\n", '
                   'sizeof(tad_job), sizeof(tad_columns), sizeof(tad_points), sizeof(tad_key_columns), sizeof(tad_drop_flow_columns), '
                   'sizeof(tad_drop_rows), TAD_FEATURE_DROP_ROWS, offsetof(tad_drop_flow_columns, keep), offsetof(tad_drop_flow_columns, memory), '
                   'offsetof(tad_drop_rows, memory)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:6] == sizes and got[6] == 1024
    assert got[7:] == [_capi.DropFlowColumns.keep.offset, _capi.DropFlowColumns.memory.offset, _capi.DropRows.memory.offset]


def test_library_exports_the_symbols_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 1024 and f & 2047 == 2047                                                    # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, with a message, and nothing is written
    cols = _capi.DropFlowColumns()
    res = ctypes.POINTER(_capi.DropRows)()
    assert lib.tad_drop_select(None, ctypes.byref(cols), 0, 0, _capi.TAD_MEM_HOST, ctypes.byref(res)) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert b"tad_drop_select: engine is NULL" in lib.tad_last_error(None)
    assert lib.tad_drop_select(None, None, 0, 0, _capi.TAD_MEM_DEVICE, None) == _capi.TAD_ERR_INVALID_ARGUMENT
    assert not res
    lib.tad_drop_rows_free(None, None)                                                      # freeing nothing is allowed


def test_the_unit_is_hip_in_its_own_source():
    from theia_amd import build
    assert "tad_drop_select.hip" in build.SOURCES
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    src = open(os.path.join(csrc, "tad_drop_select.hip")).read()
    for name in ("k_dsel_flags", "k_dsel_emit", "launch_dsel_flags", "launch_dsel_emit", "__popc", "__shfl_up", "__shared__", "__syncthreads", "uint4",
                 "code_anchor_drop_select"):
        assert name in src, name
    assert "asm" not in src and "rocprim" not in src.lower() and "hipcub" not in src.lower() and "atomic" not in src
    internal = open(os.path.join(csrc, "tad_internal.h")).read()
    assert re.search(r"constexpr int kDselLaneRows = 16;", internal) and re.search(r"constexpr int kDselTileRows = 4096;", internal)
    host = open(os.path.join(csrc, "tad_capi_ingest.cpp")).read()
    body = host[host.index("int tad_drop_select("):host.index("void tad_drop_rows_free(")]
    assert body.index("launch_dsel_flags(") < body.index("launch_scan(") < body.index("launch_dsel_emit(") and "Lease lease(eng)" in body
    assert body.count("hipStreamSynchronize(s)") == 3                                      # the total, the end (and one error path)
    assert "code_anchor_drop_select()" in open(os.path.join(csrc, "tad_engine.cpp")).read()


class _FakeLib:
    """a library of before the feature: tad_features() without the bit, and none of the calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def __getattr__(self, name):
        raise AssertionError("a wrapper touched %s on a library without TAD_FEATURE_DROP_ROWS" % name)


@pytest.mark.parametrize("lib", [_FakeLib(1023), object()], ids=["without-the-bit", "without-tad_features"])
def test_the_wrapper_raises_cleanly_without_the_feature_bit(lib):
    from theia_amd import TadEngine, TadError, _capi
    eng = TadEngine.__new__(TadEngine)
    eng._lib, eng._h = lib, None
    z8, z = np.zeros(1, np.uint8), np.zeros(1, np.int64)
    with pytest.raises(TadError) as ei:
        eng.drop_select(z8, z8, z, z, z, z, z, z, z)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_DROP_ROWS" in ei.value.message


def test_go_binding_binds_the_call_behind_its_guard():
    assert "func hasDropRows() bool" in GO and "C.tad_features()&C.TAD_FEATURE_DROP_ROWS" in GO
    fn = "func (e *Engine) DropSelect("
    body = GO[GO.index(fn):]
    body = body[:body.index("\n}\n")]
    assert body.index("hasDropRows()") < body.index("C.tad_drop_select(")
    assert not re.search(r"unsafe\.Pointer\(&\w+\[0\]\)", body)                              # no pointer into a Go slice crosses to the library
    assert "C.tad_drop_rows_free(" in GO[GO.index("func (r *DropRows) Close()"):]


def test_the_host_layers_exist_and_say_what_a_feed_must_hold():
    from theia_amd import drop_detection as dd
    assert callable(dd.drop_detection_from_flows) and hasattr(dd.PeriodicalDropDetection, "feed_flows")
    doc = " ".join(dd.PeriodicalDropDetection.feed_flows.__doc__.split())
    assert "WHOLE DAYS" in doc and "late row" in doc and "refused" in doc


# ---- the two host forms of the query agree: the two GROUP BYs compose ----
def seeded_table(seed, n, n_ip=6, n_ns=3, n_pod=5, days=4, t0=1660176000):
    """Flow rows on codes: every action value incl. both-drop pairs, pods and IPs on either side, the SAME entity seen with a pod name in
    some rows and without one in others, pod-name and IP codes that overlap numerically, several rows per (endpoint, day)."""
    rng = np.random.default_rng(seed)
    d = {"ip": ["10.0.0.%d" % i for i in range(n_ip)], "pod_ns": ["ns%d" % i for i in range(n_ns)], "pod_name": [""] + ["pod-%d" % i for i in range(1, n_pod)]}
    acts = np.array([0, 1, 2, 3, 4, 255], dtype=np.uint8)
    c = {"ingress_action": acts[rng.integers(0, 6, n)], "egress_action": acts[rng.integers(0, 6, n)]}
    for side in ("src", "dst"):
        ip = rng.integers(0, n_ip, n)
        c[side + "_ip"] = ip
        c[side + "_pod_ns"] = ip % n_ns                                   # an entity = an IP, with its namespace and pod name ...
        c[side + "_pod_name"] = np.where(rng.random(n) < 0.5, 0, 1 + ip % (n_pod - 1))     # ... which half of its rows do not carry
    c["flow_start_s"] = t0 + rng.integers(0, days * dq.DAY, n)
    c["flow_end_s"] = c["flow_start_s"] + rng.integers(0, 7200, n)
    return c, d


@pytest.mark.parametrize("seed,n,start,end,with_keep", [(1, 600, 0, 0, False), (2, 2500, 1660176000 + 40000, 0, False),
                                                        (3, 2500, 0, 1660176000 + 3 * 86400, True), (4, 4000, 1660176000 + 86400, 1660176000 + 3 * 86400 + 77, True)])
def test_the_two_reference_forms_agree_on_seeded_tables(seed, n, start, end, with_keep):
    c, d = seeded_table(seed, n)
    keep = (np.random.default_rng(seed + 100).random(n) < 0.8).astype(np.uint8) if with_keep else None
    ia, ea = c["ingress_action"], c["egress_action"]
    both = np.isin(ia, (2, 3)) & np.isin(ea, (2, 3))
    assert both.sum() > 10                                                                  # rows where both actions drop
    sel = dq.select_rows(ia, ea, c["flow_start_s"], c["src_ip"], c["src_pod_ns"], c["src_pod_name"], c["dst_ip"], c["dst_pod_ns"], c["dst_pod_name"],
                         flow_end_s=c["flow_end_s"], src_pod_null=0, dst_pod_null=0, start_time=start, end_time=end, keep=keep)
    assert np.all(sel["direction"][np.isin(sel["row"], np.flatnonzero(both))] == 0)          # ingress wins
    # endpoints seen both as pod and as IP: the same destination IP, selected once with its pod name and once without
    srow = sel["row"].astype(np.int64)
    ing_rows = srow[sel["direction"] == 0]
    as_pod = set(c["dst_ip"][ing_rows[c["dst_pod_name"][ing_rows] != 0]].tolist())
    as_ip = set(c["dst_ip"][ing_rows[c["dst_pod_name"][ing_rows] == 0]].tolist())
    assert as_pod & as_ip
    want = dq.query_pandas(dq.strings_of(c, d), ia, ea, c["flow_start_s"], c["flow_end_s"], start, end, keep)
    got = dq.sum_selected(sel, d)
    assert len(want) > 20 and int(want["dropNumber"].max()) > 1
    assert got.values.tolist() == want.values.tolist()
    assert int(got["dropNumber"].sum()) == sel["row"].size
    assert np.array_equal(sel["row"], np.sort(sel["row"]))                                  # input order
