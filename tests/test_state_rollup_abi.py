"""CPU tests of tad_state_rollup's boundary (include/tad.h: TAD_FEATURE_STATE_ROLLUP): the feature bit, the struct and the call in the
header with the words of its contract, the ctypes mirror against the compiler's layout, the exported symbol, the refusals that need no
device, the Go binding's call, the Python wrappers against a library without the bit, and the new workspace block of
theia_amd/csrc/tad_carve.h against its size function in a stand-alone program.  No compute calls."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
from job_helpers import HEADER, ROOT

CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ARGS = ["tad_engine *e", "tad_state *s", "int64_t before_t", "int64_t bucket_s", "int64_t bucket_origin", "tad_value_op bucket_op", "double ewma_alpha",
        "tad_rollup_stats *stats"]
FIELDS = ["points_before", "points_after", "points_rolled", "buckets", "keys_changed", "before_t", "ms_total", "job_context"]
BIT = 524288


def test_header_defines_the_bit_the_struct_and_the_call_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_ROLLUP\s+524288u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    m = re.search(r"\b(\w+)\s+tad_state_rollup\s*\(([^;]*?)\)\s*;", CODE, flags=re.S)
    assert m and m.group(1) == "int" and [" ".join(a.split()) for a in m.group(2).split(",")] == ARGS
    body = re.search(r"typedef struct \{([^}]*)\} tad_rollup_stats;", CODE, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == FIELDS
    section = HEADER[HEADER.index("TAD_FEATURE_STATE_ROLLUP; check tad_features()"):HEADER.index("#define TAD_FEATURE_STATE_ROLLUP")]
    for must in ("FLOORED to a bucket start", "no bucket straddles it", "bit for\n * bit", "ONE tad_run_stream EWMA batch over Wr", "idempotent", "composable",
                 "tiers commute", "keep_points counts POINTS", "accepted iff it is newer than the NEW last_t", "a later roll-up folds them",
                 "double-counts", "Atomic like a trim", "checked before any candidate is written", "tad_state_bytes falls", "stale times",
                 "TAD_OP_SUM / TAD_OP_MAX", "[0, 1]", "2^62", "TAD_OK with the state untouched", "no packed\n * copy of the state",
                 "Lock order: the state, then a job context"):
        assert must in section, must


def test_ctypes_mirror_matches_the_compilers_layout(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_ROLLUP == BIT and _capi.TAD_ABI_VERSION == 13
    S = _capi.RollupStats
    assert [n for n, _ in S._fields_] == FIELDS
    res, argtypes = _capi.SYMBOLS["tad_state_rollup"]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS) and argtypes[7] == ctypes.POINTER(S)
    assert argtypes[2:7] == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_double]
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.ReportWindow, _capi.Changes, _capi.BucketWindow)] == [136, 96, 64, 56, 88]
    probe = ["sizeof(tad_rollup_stats)"] + ["offsetof(tad_rollup_stats, %s)" % f for f in FIELDS]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("' + "%zu " * len(probe) + '%u\\n", ' + ", ".join(probe) +
                   ", TAD_FEATURE_STATE_ROLLUP); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [BIT]
    assert ctypes.sizeof(S) == 64


def test_library_exports_the_symbol_and_refuses_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_state_rollup")
    f = lib.tad_features()
    assert f & BIT and f & (BIT - 1) == BIT - 1                          # the new bit, and every earlier one
    assert lib.tad_abi_version() == 13
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    SUM = _capi.TAD_OP["sum"]
    # a NULL engine or state: TAD_ERR_INVALID_ARGUMENT whatever else is passed, nothing touched, the stats zeroed
    for args in ((1000, 60, 0, SUM, 0.0), (1000, 0, 0, SUM, 0.0), (1000, 60, 60, SUM, 0.0), (1000, 60, 0, 0, 0.0), (1000, 60, 0, SUM, 2.0), (1 << 62, 60, 0, SUM, 0.0)):
        rs = _capi.RollupStats(points_before=7, before_t=9)
        assert lib.tad_state_rollup(None, None, *args, ctypes.byref(rs)) == inv
        assert (rs.points_before, rs.before_t) == (0, 0)
        assert lib.tad_state_rollup(None, None, *args, None) == inv


def test_the_go_binding_names_the_call():
    go = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
    assert "C.tad_state_rollup(" in go and "C.tad_rollup_stats" in go and "C.TAD_FEATURE_STATE_ROLLUP" in go
    m = re.search(r"func \(s \*State\) Rollup\(before, bucketS, origin int64, op ValueOp, alpha float64\) \(RollupStats, error\)", go)
    assert m, "State.Rollup"
    body = go[go.index("type RollupStats struct"):m.start()]
    for field in ("PointsBefore", "PointsAfter", "PointsRolled", "Buckets", "KeysChanged", "BeforeT", "MsTotal", "JobContext"):
        assert re.search(r"\b%s\b" % field, body), field
    call = go[m.end():]
    for field in FIELDS:
        assert "ru.%s" % field in call[:call.index("\n}\n")], field


class _OldLib:
    """a library of before the feature: every earlier bit"""

    def tad_features(self):
        return BIT - 1

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STATE_ROLLUP" % name)


class _Engine:
    _lib = _OldLib()
    _h = None


def test_the_python_wrappers():
    from theia_amd import TadError, _capi
    from theia_amd.engine import TadState
    from theia_amd.stream_detection import StreamingAnomalyDetection
    p = inspect.signature(TadState.rollup).parameters
    assert list(p) == ["self", "before", "bucket_s", "origin", "op", "alpha"]
    assert (p["origin"].default, p["op"].default, p["alpha"].default) == (0, "sum", 0.0)
    q = inspect.signature(StreamingAnomalyDetection.rollup).parameters
    assert list(q) == ["self", "before", "bucket_s", "bucket_op"] and q["bucket_op"].default == "sum"
    st = object.__new__(TadState)
    st._engine, st._h = _Engine(), None
    with pytest.raises(TadError) as ei:
        st.rollup(1000, 60)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_ROLLUP" in str(ei.value)


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "tad_carve.h"
using namespace tad;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
typedef unsigned char u8;

// rollup_keys_layout over a sweep of keys x chunks: the measuring walk and the placing walk end at the same byte count, that count is the
// formula of its parts, every array lies inside the block and touches no other, none starts off its 16 bytes, the guards stay intact
int main() {
  long blocks = 0;
  constexpr size_t kGuard = 64;
  static_assert(sizeof(RollupCounters) == 64, "one 64-byte block");
  for (uint64_t K : {1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025})
    for (uint64_t chunks : {K + 1, K + 2, K + 5, K + 64, K + 1000}) {
      const size_t kpad = (size_t)((K + 3) & ~3ull), cpad = (size_t)((chunks + 3) & ~3ull);
      const size_t want = 64 + 5 * kpad * 4 + 64 + (kpad + 4) * 8 + cpad * 4 + (cpad + 4) * 8;
      Carve m(nullptr);
      const RollupKeys none = rollup_keys_layout(m, K, chunks);
      CHECK(m.bytes() == want && !m.misaligned());
      CHECK(!none.rc && !none.beg && !none.len && !none.rcnt && !none.ecnt && !none.chunks && !none.long_count && !none.coff && !none.hcnt && !none.hoff);
      const size_t total = (want + 2 * kGuard + 511) / 256 * 256 + 256;
      u8 *raw = static_cast<u8 *>(aligned_alloc(256, total));
      CHECK(raw != nullptr);
      memset(raw, 0xEE, total);
      u8 *base = raw + 256;
      Carve c(base);
      const RollupKeys r = rollup_keys_layout(c, K, chunks);
      CHECK(c.bytes() == want && !c.misaligned());
      CHECK(reinterpret_cast<u8 *>(r.rc) == base);
      CHECK(reinterpret_cast<u8 *>(r.beg) == base + 64);
      CHECK(r.len == r.beg + kpad && r.rcnt == r.len + kpad && r.ecnt == r.rcnt + kpad && r.chunks == r.ecnt + kpad);
      CHECK(reinterpret_cast<u8 *>(r.long_count) == reinterpret_cast<u8 *>(r.chunks + kpad));
      CHECK(reinterpret_cast<u8 *>(r.coff) == reinterpret_cast<u8 *>(r.long_count) + 64);
      CHECK(reinterpret_cast<u8 *>(r.hcnt) == reinterpret_cast<u8 *>(r.coff + kpad + 4));
      CHECK(reinterpret_cast<u8 *>(r.hoff) == reinterpret_cast<u8 *>(r.hcnt + cpad));
      CHECK(reinterpret_cast<u8 *>(r.hoff + cpad + 4) == base + want);
      CHECK(kpad + 4 >= K + 1 && cpad + 4 >= chunks + 1);          // the offset arrays hold their last entry
      struct { void *p; size_t n; } parts[10] = {{r.rc, 64}, {r.beg, kpad * 4}, {r.len, kpad * 4}, {r.rcnt, kpad * 4}, {r.ecnt, kpad * 4},
                                                 {r.chunks, kpad * 4}, {r.long_count, 64}, {r.coff, (kpad + 4) * 8}, {r.hcnt, cpad * 4},
                                                 {r.hoff, (cpad + 4) * 8}};
      for (int i = 0; i < 10; ++i) CHECK(reinterpret_cast<uintptr_t>(parts[i].p) % 16 == 0);
      for (int i = 0; i < 10; ++i) memset(parts[i].p, i + 1, parts[i].n);
      for (int i = 0; i < 10; ++i)
        for (size_t j = 0; j < parts[i].n; ++j) CHECK(static_cast<u8 *>(parts[i].p)[j] == (u8)(i + 1));   // no later array wrote into this one
      for (size_t j = 0; j < kGuard; ++j) CHECK(base[-(long)j - 1] == 0xEE && base[want + j] == 0xEE);
      free(raw);
      ++blocks;
    }
  printf("blocks %ld\n", blocks);
  return 0;
}
"""


def test_the_rollup_workspace_block_measures_what_it_places(tmp_path):
    src = tmp_path / "rollup_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "rollup_layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "blocks 55" in r.stdout, r.stdout + r.stderr
