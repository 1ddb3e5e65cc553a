"""CPU tests of tad_state_replace's boundary (include/tad.h: TAD_FEATURE_STATE_REPLACE): the feature bit and the declaration in the header,
the contract's words, the ctypes mirror against the compiler's layout, the exported symbol, tad_features() and the refusals that need no
device, the kernels' source, the Python wrapper against a library without the bit, stream_rows_query's SQL for each mode, and
StreamingAnomalyDetection.poll against the in-process ClickHouse stand-in of tests/test_clickhouse_http.py.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from theia_amd import clickhouse as ch
from fake_clickhouse import arrow_table, server  # noqa: F401  (server: the fixture)
from job_helpers import HEADER, ROOT

CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_columns *cols", "uint32_t flags", "int64_t from_t", "int64_t to_t",
        "int64_t keep_from_t", "tad_replace_stats *stats"]
STATS_FIELDS = ["rows_in", "rows_used", "batch_points", "points_too_old", "points_appended", "points_inserted", "points_replaced", "points_erased",
                "keys_emptied", "keys_touched", "keys_replayed", "stage0_path", "stage0_attempts", "job_context", "reserved", "ms_stage0", "ms_replace",
                "ms_total", "reserved1"]


def test_header_defines_the_bit_the_flag_and_the_call_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_REPLACE\s+65536u\b", HEADER)
    assert re.search(r"#define\s+TAD_REPLACE_RANGE\s+1u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    proto = re.search(r"\b(\w+)\s+tad_state_replace\s*\(([^;]*?)\)\s*;", CODE, flags=re.S)
    assert proto and proto.group(1) == "int"
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == ARGS
    body = re.search(r"typedef struct \{([^}]*)\} tad_replace_stats;", CODE, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == STATS_FIELDS


def test_header_states_the_contract_under_the_merge_and_corrects_its_sentence():
    start = HEADER.index("TAD_FEATURE_STATE_REPLACE; check tad_features()")
    assert HEADER.index("int tad_state_merge(") < start < HEADER.index("int tad_state_replace(") < HEADER.index("int tad_run_state_window(")
    section = HEADER[start:HEADER.index("int tad_state_replace(")]
    for must in ("pure function of W", "without the points whose flow_end_s < keep_from_t", "empty without TAD_REPLACE_RANGE", "half-open",
                 "from_t = to_t = 0 is", "not in R", "ONE tad_run_stream EWMA batch over W'", "the same call twice leaves the same bits",
                 "never combined", "becomes an unseen key", "EVERY key of the state", "only aggregates rows inside the batch", "unknown bits in flags",
                 "without TAD_REPLACE_RANGE", "from_t > to_t", "from_t == to_t non-zero is an empty R", "TAD_ERR_KEY_RANGE", "leaves the state as it was",
                 "is not a no-op", "keys_replayed == 0", "a quarter of its capacity", "Lock order: the state, then a job context"):
        assert must in section, must
    for other in re.findall(r"TAD_FEATURE_\w+; check tad_features\(\)", HEADER):
        assert HEADER.count(other) == 1, other
    assert not re.search(r"\bint tad_\w+\(", section)
    merge = HEADER[HEADER.index("TAD_FEATURE_STATE_MERGE; check tad_features()"):HEADER.index("int tad_state_merge(")]
    assert "doubles the values under sum" in merge and "tad_state_replace" in merge


def test_ctypes_mirror_matches_the_compilers_layout(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_REPLACE == 65536 and _capi.TAD_REPLACE_RANGE == 1 and _capi.TAD_ABI_VERSION == 13
    res, argtypes = _capi.SYMBOLS["tad_state_replace"]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS)
    assert argtypes[4] is ctypes.c_uint32 and argtypes[5:8] == [ctypes.c_int64] * 3 and argtypes[8] == ctypes.POINTER(_capi.ReplaceStats)
    S = _capi.ReplaceStats
    assert [n for n, _ in S._fields_] == STATS_FIELDS
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.MergeStats, _capi.CompactStats)] == [136, 96, 104, 96]
    probe = ["sizeof(tad_replace_stats)"] + ["offsetof(tad_replace_stats, %s)" % f for f in STATS_FIELDS]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("' + "%zu " * len(probe) + '\\n", ' + ", ".join(probe) +
                   "); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in STATS_FIELDS]
    assert ctypes.sizeof(S) == 120


def test_library_exports_the_symbol_and_refuses_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_state_replace")
    f = lib.tad_features()
    assert f & 65536 and f & 65535 == 65535              # the new bit, and every earlier one
    assert lib.tad_abi_version() == 13
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    stats = _capi.ReplaceStats()
    ctypes.memset(ctypes.byref(stats), 0x5A, ctypes.sizeof(stats))
    job, cols = _capi.Job(), _capi.Columns()
    # a NULL engine: refused before anything is touched, the stats zeroed as tad_state_merge zeroes its own
    assert lib.tad_state_replace(None, None, ctypes.byref(job), ctypes.byref(cols), 0, 0, 0, 0, ctypes.byref(stats)) == inv
    assert bytes(stats) == bytes(ctypes.sizeof(stats))
    assert lib.tad_state_replace(None, None, None, None, _capi.TAD_REPLACE_RANGE, 5, 3, 0, None) == inv


def test_the_kernels_are_hip_in_a_unit_of_their_own_beside_the_merge():
    """(the name is of before the merge and the replace shared their kernels: the unit is the merge's, tad_merge.hip)"""
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    assert not os.path.exists(os.path.join(csrc, "tad_replace.hip"))
    src = open(os.path.join(csrc, "tad_merge.hip")).read()
    for name in ("k_merge_range", "k_merge_keys", "k_merge_series", "launch_merge_range", "launch_merge_keys", "launch_merge_series",
                 "code_anchor_merge", "kMergeChunk = 2048", "static_assert(kMergeChunk == kHistChunk"):
        assert name in src, name
    assert "__shared__" not in src and not re.search(r"\basm\b|__asm", src) and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src) == ["stdint.h", "tad_internal.h"]
    from theia_amd import build
    assert "tad_merge.hip" in build.SOURCES and "tad_replace.hip" not in build.SOURCES
    host = open(os.path.join(csrc, "tad_capi.cpp")).read()
    assert "state_replace_batch" not in host                                         # one driver
    body = host[host.index("int state_merge_batch("):host.index("constexpr uint64_t kStreamFitWaves")]
    # one classification, one set of scans, history kernels and moments; the erased total is read before anything is written
    order = ["state_grow_candidates(", "launch_merge_classify(", "launch_merge_range(", "append_batch(", "state_size_arenas(", "launch_merge_keys(",
             "launch_merge_series(", "launch_hist_sort(", "launch_hist_subtract(", "launch_hist_merge(", "launch_merge_moments("]
    at = [body.index(x) for x in order]
    assert at == sorted(at), list(zip(order, at))
    assert "int tad_state_replace(" in host and "replace_keys_layout" in open(os.path.join(csrc, "tad_carve.h")).read()
    # the merge still combines, the replace assigns the batch's value; a range only comes with the replace rule
    assert "if constexpr (RULE == MERGE_SUM) return x + y;" in src
    assert "else if constexpr (RULE == MERGE_MAX) return x > y ? x : y;" in src
    assert "else return y;" in src
    assert "x = merge_value<RULE>(x, nv[j]);" in src and "hadd[aoff[j]] = merge_value<RULE>(x, y);" in src
    assert "static_assert(!RANGED || RULE == MERGE_REPLACE" in src
    for inst in ("<MERGE_SUM, false>", "<MERGE_MAX, false>", "<MERGE_REPLACE, false>", "<MERGE_REPLACE, true>"):
        assert src.count("launch_series_as" + inst) == 1, inst


class _OldLib:
    """a library of before the feature: every earlier bit"""

    def tad_features(self):
        return 65535

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STATE_REPLACE" % name)


def test_replace_stream_refuses_a_library_without_the_bit():
    from theia_amd import TadError, _capi
    from theia_amd.engine import TadEngine
    eng = object.__new__(TadEngine)
    eng._lib = _OldLib()
    with pytest.raises(TadError) as ei:
        eng.replace_stream(None, np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint64))
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_REPLACE" in str(ei.value)


# ---- the streaming feed's query ----
def test_stream_rows_query_for_each_mode():
    q = ch.stream_rows_query
    assert q("svc", "labels", (), 100, 200) == (
        "SELECT destinationServicePortName, flowEndSeconds, throughput FROM default.flows WHERE destinationServicePortName <> '' "
        "AND flowEndSeconds >= toDateTime(100) AND flowEndSeconds < toDateTime(200)")
    assert q("external", "labels", ["kube-system", "infra"], 100, 200) == (
        "SELECT destinationIP, flowType, sourcePodNamespace, destinationPodNamespace, flowEndSeconds, throughput FROM default.flows WHERE "
        "sourcePodNamespace NOT IN ('kube-system', 'infra') AND destinationPodNamespace NOT IN ('kube-system', 'infra') AND flowType = 3 "
        "AND flowEndSeconds >= toDateTime(100) AND flowEndSeconds < toDateTime(200)")
    assert q("pod", "labels", (), 100, 200) == (
        "SELECT sourcePodNamespace, destinationPodNamespace, sourcePodLabels, destinationPodLabels, flowEndSeconds, throughput FROM default.flows WHERE "
        "(destinationPodLabels <> '' OR sourcePodLabels <> '') AND flowEndSeconds >= toDateTime(100) AND flowEndSeconds < toDateTime(200)")
    assert q("pod", "name", (), 0, 200) == (
        "SELECT sourcePodNamespace, destinationPodNamespace, sourcePodName, destinationPodName, flowEndSeconds, throughput FROM default.flows WHERE "
        "(destinationPodName <> '' OR sourcePodName <> '') AND flowEndSeconds < toDateTime(200)")
    d = q("svc", "labels", (), 100, 200, dictionary=True)
    assert d.startswith("SELECT toLowCardinality(destinationServicePortName) AS destinationServicePortName, flowEndSeconds, throughput FROM default.flows")
    for mode in ("svc", "external", "pod"):
        sql = q(mode, "labels", ["kube-system"], 1, 2)
        assert "flowStartSeconds" not in sql and "ilike" not in sql and "destinationIP =" not in sql and "GROUP BY" not in sql
        assert ch.stream_rows_columns(mode, "labels", ["kube-system"]) == sql[len("SELECT "):sql.index(" FROM ")].split(", ")
    with pytest.raises(ValueError):
        q("", "labels", (), 1, 2)
    with pytest.raises(ValueError):
        q("pod", "uid", (), 1, 2)
    # rows_query stays as it is
    assert ch.rows_query("", "2022-08-11 08:00:00", [], "svc") == (
        "SELECT destinationServicePortName, flowStartSeconds, flowEndSeconds, throughput, sourcePodNamespace, destinationPodNamespace FROM default.flows "
        "WHERE flowEndSeconds < '2022-08-11 08:00:00' AND destinationServicePortName <> ''")


# ---- the poll loop against the ClickHouse stand-in ----


def _instance(mode, ident="labels", ignore=()):
    """a StreamingAnomalyDetection without a device: what poll itself uses, with the feed recorded"""
    from theia_amd.stream_detection import StreamingAnomalyDetection
    s = object.__new__(StreamingAnomalyDetection)
    s.agg_flow, s.pod_ident, s.ns_ignore_list, s.watermark, s._broken = mode, ident, tuple(ignore), 0, None
    s.fed = []
    s.feed = lambda flows, replace=None: s.fed.append((flows, replace)) or {"points_replaced": 0}
    return s


def test_poll_reads_the_lagged_range_feeds_it_with_replace_and_moves_the_watermark(server, monkeypatch):
    monkeypatch.delenv("CLICKHOUSE_USERNAME", raising=False)
    client = ch.ClickHouseHTTP(server.url)
    s = _instance("svc")
    rows = {"destinationServicePortName": np.array(["a/b:c", "", "a/b:c"]), "flowEndSeconds": np.array([1000, 1010, 1020], np.int64),
            "throughput": np.array([5, 6, 1 << 63], np.uint64)}
    first = ch.stream_rows_query("svc", "labels", [], 0, 1100)
    assert "flowEndSeconds >=" not in first               # the first turn reads everything before `now`
    server.responses[first] = arrow_table(rows)
    assert s.poll(client, 1100, 60) == {"points_replaced": 0}
    flows, rep = s.fed[-1]
    assert rep == (0, 1100) and s.watermark == 1100
    assert np.asarray(flows["flowEndSeconds"]).astype(np.int64).tolist() == [1000, 1010, 1020]
    assert flows["throughput"].dtype == np.uint64 and int(flows["throughput"][2]) == 1 << 63
    assert [str(x) for x in np.asarray(flows["destinationServicePortName"] if not hasattr(flows["destinationServicePortName"], "materialise")
                                       else flows["destinationServicePortName"].materialise())] == ["a/b:c", "", "a/b:c"]
    # the second turn re-reads the lag; an empty answer is still fed, so that the range is erased
    second = ch.stream_rows_query("svc", "labels", [], 1040, 1200)
    server.responses[second] = arrow_table({k: v[:0] for k, v in rows.items()})
    s.poll(client, 1200, 60)
    flows, rep = s.fed[-1]
    assert rep == (1040, 1200) and s.watermark == 1200
    assert set(flows) == {"destinationServicePortName", "flowEndSeconds", "throughput"} and len(flows["flowEndSeconds"]) == 0
    assert [q[:-len(" FORMAT ArrowStream")] for q in server.queries] == [first, second]
    # a turn that does not move forward, or a negative lag, is refused before any read
    with pytest.raises(ValueError):
        s.poll(client, 1100, 60)
    with pytest.raises(ValueError):
        s.poll(client, 1300, -1)
    assert len(server.queries) == 2 and s.watermark == 1200


def test_poll_sends_the_instances_mode_and_ignore_list(server, monkeypatch):
    monkeypatch.delenv("CLICKHOUSE_USERNAME", raising=False)
    client = ch.ClickHouseHTTP(server.url)
    s = _instance("pod", "name", ["kube-system"])
    s.watermark = 5000
    sql = ch.stream_rows_query("pod", "name", ["kube-system"], 4700, 5600)
    server.responses[sql] = arrow_table({"sourcePodNamespace": np.array(["a"]), "destinationPodNamespace": np.array(["b"]), "sourcePodName": np.array(["p"]),
                                         "destinationPodName": np.array([""]), "flowEndSeconds": np.array([5000], np.int64),
                                         "throughput": np.array([7], np.uint64)})
    s.poll(client, 5600, 300)
    assert s.fed[-1][1] == (4700, 5600) and server.queries[-1].startswith(sql)


def test_the_two_workspace_layouts_measure_what_they_place(tmp_path):
    """replace_keys_layout / replace_loss_layout (tad_carve.h) in a stand-alone host program: the measuring walk and the placing walk agree,
    no array starts off its alignment, the arrays do not overlap and the block ends where the last one ends"""
    src = tmp_path / "layout.cpp"
    src.write_text(r'''
#include <stdio.h>
#include <stdlib.h>
#include "tad_carve.h"
using namespace tad;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
  const unsigned long long Ks[] = {0, 1, 3, 4, 5, 63, 64, 65, 1000, 100003};
  for (unsigned long long K : Ks) {
    Carve m(nullptr);
    replace_keys_layout(m, K);
    unsigned char *b = static_cast<unsigned char *>(aligned_alloc(64, m.bytes() + 64));
    Carve c(b);
    const ReplaceKeys r = replace_keys_layout(c, K);
    const size_t kp = kpad4(K);
    CHECK(c.bytes() == m.bytes() && !c.misaligned() && !m.misaligned());
    CHECK((unsigned char *)r.ebeg == b && r.eend == r.ebeg + kp && r.ecnt == r.eend + kp);
    CHECK((unsigned char *)r.eoff == (unsigned char *)(r.ecnt + kp) && r.pzero == r.eoff + kp + 4);
    CHECK((unsigned char *)(r.pzero + kp + 4) == b + c.bytes() && kp >= K && kp + 4 >= K + 1);
    CHECK(((size_t)((unsigned char *)r.eoff - b)) % 16 == 0);
    free(b);
  }
  const unsigned long long ns[] = {1, 2, 7, 4096, 1000001};
  for (unsigned long long n : ns) {
    Carve m(nullptr);
    replace_loss_layout(m, n);
    unsigned char *b = static_cast<unsigned char *>(aligned_alloc(64, m.bytes() + 64));
    Carve c(b);
    const ReplaceLoss l = replace_loss_layout(c, n);
    CHECK(c.bytes() == m.bytes() && m.bytes() == n * 16 && !c.misaligned());
    CHECK((unsigned char *)l.hrem == b && l.hrem_s == l.hrem + n);
    free(b);
  }
  printf("ok\n");
  return 0;
}
''')
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "theia_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
