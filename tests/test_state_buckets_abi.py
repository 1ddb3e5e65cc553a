"""CPU tests of tad_run_state_buckets' boundary (include/tad.h: TAD_FEATURE_STATE_BUCKETS): the feature bit, the struct and the call in the
header, the ctypes mirror against the compiler's layout, the exported symbol, the refusals that need no device, the Go binding's call, the
Python wrappers against a library without the bit, and the new workspace block of theia_amd/csrc/tad_carve.h against its size function in a
stand-alone program (tests/test_workspace_layout.py's checks for the one new layout).  No compute calls."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
from job_helpers import HEADER, ROOT

CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ARGS = ["tad_engine *e", "tad_state *s", "const tad_job *job", "const tad_bucket_window *w", "tad_mem out_memory", "tad_result **out"]
FIELDS = ["from_t", "to_t", "keep_points", "key_keep", "key_since", "since_t", "num_keys", "key_memory", "bucket_s", "bucket_origin", "bucket_op"]


def _proto(name):
    m = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert m and m.group(1) == "int", name
    return [" ".join(a.split()) for a in m.group(2).split(",")]


def test_header_defines_the_bit_the_struct_and_the_call_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STATE_BUCKETS\s+262144u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    assert _proto("tad_run_state_buckets") == ARGS
    body = re.search(r"typedef struct \{([^}]*)\} tad_bucket_window;", CODE, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == FIELDS
    assert re.search(r"tad_value_op\s+bucket_op;", body)
    section = HEADER[HEADER.index("TAD_FEATURE_STATE_BUCKETS; check tad_features()"):HEADER.index("#define TAD_FEATURE_STATE_BUCKETS")]
    for must in ("floor((flow_end_s - bucket_origin) / bucket_s)", "FLOOR division", "applied FIRST", "bit for bit", "IS the *_keys call", "Read-only",
                 "reported iff its start >=", "reported, whole", "TAD_NO_CHANGE deselects", "bucket_s < 1", "outside [0, bucket_s)", "TAD_OP_AUTO too",
                 "TAD_ALGO_DROP", "rows_in = rows_used = the window's RAW points", "n_points = the buckets", "host_syncs", "2^62", "2^40",
                 "no\n * unbucketed copy of the window is written", "16 B per bucket"):
        assert must in section, must
    assert "tad_drop_state_buckets" not in CODE


def test_ctypes_mirror_matches_the_compilers_layout(tmp_path):
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STATE_BUCKETS == 262144 and _capi.TAD_ABI_VERSION == 13
    S = _capi.BucketWindow
    assert [n for n, _ in S._fields_] == FIELDS
    res, argtypes = _capi.SYMBOLS["tad_run_state_buckets"]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS) and argtypes[3] == ctypes.POINTER(S)
    assert argtypes[:3] + argtypes[4:] == _capi.SYMBOLS["tad_run_state_since"][1][:3] + _capi.SYMBOLS["tad_run_state_since"][1][4:]
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.ReportWindow, _capi.Changes)] == [136, 96, 64, 56]
    probe = ["sizeof(tad_bucket_window)"] + ["offsetof(tad_bucket_window, %s)" % f for f in FIELDS]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tad.h"\nint main(void) { printf("' + "%zu " * len(probe) + '%u\\n", ' + ", ".join(probe) +
                   ", TAD_FEATURE_STATE_BUCKETS); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [262144]
    assert ctypes.sizeof(S) == 88
    # the first eight fields are tad_report_window's, at its offsets
    for f in FIELDS[:8]:
        assert getattr(S, f).offset == getattr(_capi.ReportWindow, f).offset, f


def test_library_exports_the_symbol_and_refuses_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_run_state_buckets")
    f = lib.tad_features()
    assert f & 262144 and f & 131072 and f & 131071 == 131071           # the new bit, and every earlier one
    assert lib.tad_abi_version() == 13
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    job = _capi.Job()
    res = ctypes.POINTER(_capi.Result)()
    S = _capi.BucketWindow
    good = dict(bucket_s=60, bucket_origin=0, bucket_op=_capi.TAD_OP["sum"])
    # a NULL engine: TAD_ERR_INVALID_ARGUMENT whatever else is passed, nothing touched
    for w in (S(**good), S(bucket_s=0), S(bucket_s=60, bucket_origin=60, bucket_op=2), S(bucket_s=60, bucket_op=0), S(since_t=5, **good)):
        assert lib.tad_run_state_buckets(None, None, ctypes.byref(job), ctypes.byref(w), 0, ctypes.byref(res)) == inv and not res
    assert lib.tad_run_state_buckets(None, None, ctypes.byref(job), None, 0, ctypes.byref(res)) == inv
    assert lib.tad_run_state_buckets(None, None, None, None, 0, None) == inv


def test_the_go_binding_names_the_call():
    go = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
    assert "C.tad_run_state_buckets(" in go and "C.tad_bucket_window" in go and "C.TAD_FEATURE_STATE_BUCKETS" in go
    m = re.search(r"func \(s \*State\) RunBuckets\(job Job, w BucketWindow\) \(\[\]Row, error\)", go)
    assert m, "State.RunBuckets"
    for field in ("BucketS", "Origin", "Op"):
        assert re.search(r"\b%s\b" % field, go[go.index("type BucketWindow struct"):m.start()]), field


class _OldLib:
    """a library of before the feature: every earlier bit"""

    def tad_features(self):
        return 262143

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STATE_BUCKETS" % name)


class _State:
    num_keys = 3


def test_the_python_wrappers():
    from theia_amd import TadError, _capi
    from theia_amd.engine import TadEngine
    from theia_amd.stream_detection import StreamingAnomalyDetection
    p = list(inspect.signature(TadEngine.run_state_buckets).parameters)
    assert p[:11] == ["self", "state", "bucket_s", "origin", "op", "from_t", "to_t", "keep_points", "key_keep", "key_since", "since_t"] and "algo" in p
    for fn in (StreamingAnomalyDetection.job, StreamingAnomalyDetection.feed_alerts, StreamingAnomalyDetection.poll_alerts):
        sig = inspect.signature(fn).parameters
        assert sig["bucket_s"].default == 0 and sig["bucket_op"].default == "sum", fn
    assert inspect.signature(StreamingAnomalyDetection.job).parameters["complete_before"].default is None
    eng = object.__new__(TadEngine)
    eng._lib = _OldLib()
    with pytest.raises(TadError) as ei:
        eng.run_state_buckets(_State(), 60)
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STATE_BUCKETS" in str(ei.value)


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "tad_carve.h"
using namespace tad;

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
typedef unsigned char u8;

// bucket_keys_layout over a sweep of keys x chunks: the measuring walk and the placing walk end at the same byte count, that count is the
// formula of its parts, every array lies inside the block and touches no other, none starts off its 16 bytes, the guards stay intact
int main() {
  long blocks = 0;
  constexpr size_t kGuard = 64;
  for (uint64_t K : {1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025})
    for (uint64_t chunks : {K + 1, K + 2, K + 5, K + 64, K + 1000}) {
      const size_t kpad = (size_t)((K + 3) & ~3ull), cpad = (size_t)((chunks + 3) & ~3ull);
      const size_t want = kpad * 8 + (kpad + 4) * 8 + cpad * 4 + (cpad + 4) * 8;
      Carve m(nullptr);
      const BucketKeys none = bucket_keys_layout(m, K, chunks);
      CHECK(m.bytes() == want && !m.misaligned());
      CHECK(!none.bcnt && !none.becnt && !none.boff && !none.hcnt && !none.hoff);
      u8 *raw = static_cast<u8 *>(aligned_alloc(256, (want + 2 * kGuard + 511) / 256 * 256 + 256));
      CHECK(raw != nullptr);
      memset(raw, 0xEE, (want + 2 * kGuard + 511) / 256 * 256 + 256);
      u8 *base = raw + 256;
      Carve c(base);
      const BucketKeys b = bucket_keys_layout(c, K, chunks);
      CHECK(c.bytes() == want && !c.misaligned());
      CHECK(reinterpret_cast<u8 *>(b.bcnt) == base);
      CHECK(b.becnt == b.bcnt + kpad);
      CHECK(reinterpret_cast<u8 *>(b.boff) == reinterpret_cast<u8 *>(b.becnt + kpad));
      CHECK(reinterpret_cast<u8 *>(b.hcnt) == reinterpret_cast<u8 *>(b.boff + kpad + 4));
      CHECK(reinterpret_cast<u8 *>(b.hoff) == reinterpret_cast<u8 *>(b.hcnt + cpad));
      CHECK(reinterpret_cast<u8 *>(b.hoff + cpad + 4) == base + want);
      CHECK(kpad + 4 >= K + 1 && cpad + 4 >= chunks + 1);          // the offset arrays hold their last entry
      struct { void *p; size_t n; } parts[5] = {{b.bcnt, kpad * 4}, {b.becnt, kpad * 4}, {b.boff, (kpad + 4) * 8}, {b.hcnt, cpad * 4}, {b.hoff, (cpad + 4) * 8}};
      for (int i = 0; i < 5; ++i) CHECK(reinterpret_cast<uintptr_t>(parts[i].p) % 16 == 0);
      for (int i = 0; i < 5; ++i) memset(parts[i].p, i + 1, parts[i].n);
      for (int i = 0; i < 5; ++i)
        for (size_t j = 0; j < parts[i].n; ++j) CHECK(static_cast<u8 *>(parts[i].p)[j] == (u8)(i + 1));   // no later array wrote into this one
      for (size_t j = 0; j < kGuard; ++j) CHECK(base[-(long)j - 1] == 0xEE && base[want + j] == 0xEE);
      free(raw);
      ++blocks;
    }
  printf("blocks %ld\n", blocks);
  return 0;
}
"""


def test_the_bucket_workspace_block_measures_what_it_places(tmp_path):
    src = tmp_path / "bucket_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "bucket_layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "blocks 55" in r.stdout, r.stdout + r.stderr
