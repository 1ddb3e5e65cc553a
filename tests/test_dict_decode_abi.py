"""CPU tests of the decode side's boundary (include/tad.h: TAD_FEATURE_DICT_DECODE, tad_keydict_gather, tad_strdict_decode): the feature bit
and the prototypes in the header, the section's place, the ctypes mirror, the exported symbols, tad_features() and the NULL refusals without
a device, the kernels' source, the Python wrappers against a library without the bit, the Go binding's guard, and the two workspace
layouts in a stand-alone host program.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

PROTOTYPES = {
    "tad_keydict_gather": ("int", ["tad_engine *e", "const tad_keydict *d", "const uint64_t *key_id", "uint64_t n", "tad_mem memory", "int64_t *const *cols",
                                   "uint8_t *side"]),
    "tad_strdict_decode": ("int", ["tad_engine *e", "const tad_strdict *d", "const int64_t *codes", "uint64_t n", "tad_mem codes_memory", "int64_t *offsets",
                                   "uint8_t *data", "uint64_t data_cap", "tad_mem out_memory", "uint64_t *data_bytes"]),
}
GO_METHODS = {"tad_keydict_gather": "func (d *KeyDict) Gather(", "tad_strdict_decode": "func (d *StringDict) Decode("}


def test_header_defines_the_feature_bit_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_DICT_DECODE\s+8192u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_header_declares_both_calls_with_their_exact_arguments(name):
    ret, want = PROTOTYPES[name]
    proto = re.search(r"\b(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, CODE, flags=re.S)
    assert proto, "%s is not declared" % name
    assert proto.group(1) == ret
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == want


def test_header_documents_the_contract_between_the_match_call_and_the_progress_call():
    start = HEADER.index("TAD_FEATURE_DICT_DECODE; check tad_features()")
    assert HEADER.index("int tad_strdict_match(") < start < HEADER.index("int tad_keydict_gather(") < HEADER.index("int tad_strdict_decode(") < HEADER.index("int tad_progress(")
    section = HEADER[start:HEADER.index("int tad_keydict_gather(")]
    for must in ("ARBITRARY", "any order", "NULL entry skips", "TAD_KEY_SKIP", "unspecified", "One launch", "TAD_ERR_GRID_TOO_LARGE", "workspace_limit",
                 "offsets[n + 1]", "codes_memory", "out_memory", "size query", "nothing written", "TAD_CODE_NONE", "before any byte is copied", "any byte alignment",
                 "n < 2^32 - 1", "64 bits", "LDS", "The ABI stays 13", "Lock order: the dictionary, then a job context"):
        assert must in section, must
    # the section quotes no earlier prototype and no earlier section's phrase: the older tests find theirs by the first occurrence
    for other in re.findall(r"TAD_FEATURE_\w+; check tad_features\(\)", HEADER):
        assert HEADER.count(other) == 1, other
    assert not re.search(r"\bint tad_\w+\(", section)


def test_ctypes_symbols_and_the_constants():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_DICT_DECODE == 8192 and _capi.TAD_ABI_VERSION == 13
    for name, (_, args) in PROTOTYPES.items():
        res, argtypes = _capi.SYMBOLS[name]
        assert len(argtypes) == len(args), name
        assert res is ctypes.c_int, name
    assert _capi.SYMBOLS["tad_keydict_gather"][1][5] == ctypes.POINTER(ctypes.c_void_p)
    assert _capi.SYMBOLS["tad_strdict_decode"][1][9] == ctypes.POINTER(ctypes.c_uint64)
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.KeyColumns, _capi.StringColumn)] == [136, 96, 56, 64]


def test_library_exports_the_symbols_and_refuses_a_null_engine_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    for name in PROTOTYPES:
        assert hasattr(lib, name), name
    f = lib.tad_features()
    assert f & 8192 and f & _capi.TAD_FEATURE_DICT_DECODE
    assert f & 8191 == 8191                                                                 # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    ids = np.arange(4, dtype=np.uint64)
    col = np.full(4, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    side = np.full(4, 0x5A, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * 1)(col.ctypes.data)
    for mem in (_capi.TAD_MEM_HOST, _capi.TAD_MEM_DEVICE):
        assert lib.tad_keydict_gather(None, None, ids.ctypes.data, 4, mem, ptrs, side.ctypes.data) == inv
    assert (col == 0x5A5A5A5A5A5A5A5A).all() and (side == 0x5A).all()
    codes = np.arange(4, dtype=np.int64)
    offsets = np.full(5, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    data = np.full(64, 0x5A, dtype=np.uint8)
    need = ctypes.c_uint64(77)
    assert lib.tad_strdict_decode(None, None, codes.ctypes.data, 4, _capi.TAD_MEM_HOST, offsets.ctypes.data, data.ctypes.data, 64, _capi.TAD_MEM_HOST,
                                  ctypes.byref(need)) == inv
    assert lib.tad_strdict_decode(None, None, None, 0, _capi.TAD_MEM_HOST, None, None, 0, _capi.TAD_MEM_HOST, ctypes.byref(need)) == inv
    assert need.value == 77 and (offsets == 0x5A5A5A5A5A5A5A5A).all() and (data == 0x5A).all()


def test_the_kernels_are_hip_in_the_dictionaries_own_units():
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    kd = open(os.path.join(csrc, "tad_keydict.hip")).read()
    sd = open(os.path.join(csrc, "tad_strdict.hip")).read()
    internal = open(os.path.join(csrc, "tad_internal.h")).read()
    for name in ("k_kd_gather", "launch_kd_gather", "kd_load_record(keys, id, pairs, w)"):
        assert name in kd, name
    for name in ("k_sd_decode_lens", "k_sd_decode", "launch_sd_decode_lens", "launch_sd_decode", "__shared__", "sd_shifted_words"):
        assert name in sd, name
    assert re.search(r"kSdDecodeRows = 256, kSdDecodeStage = 16 \* 1024, kSdDecodeMaxBlocks = 2048;", internal)
    for src in (kd, sd):
        assert not re.search(r"\basm\b|__asm", src) and "rocprim" not in src.lower() and "hipcub" not in src.lower()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", kd) == ["tad_internal.h", "tad_slots.h"]
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", sd) == ["tad_internal.h", "tad_strbytes.h"]
    # the entry points sit with their dictionaries' host sides, the lengths go through the project's scan
    assert "int tad_keydict_gather(" in open(os.path.join(csrc, "tad_capi_keydict.cpp")).read()
    host = open(os.path.join(csrc, "tad_capi_strdict.cpp")).read()
    body = host[host.index("int tad_strdict_decode("):]
    assert body.index("launch_sd_decode_lens(") < body.index("launch_scan(") < body.index("SD_FLAG_BAD_CODE") < body.index("launch_sd_decode(s")


class _FakeLib:
    """a library of before the feature: every earlier bit, and none of the two calls"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def tad_keydict_create(self, eng, n_cols, expected, out):
        return 0

    def tad_strdict_create(self, eng, values, nbytes, out):
        return 0

    def tad_keydict_destroy(self, eng, h):
        pass

    def tad_strdict_destroy(self, eng, h):
        pass

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_DICT_DECODE" % name)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        assert rc == 0


def test_the_wrappers_ask_for_the_bit_when_called_not_when_constructed():
    from theia_amd import KeyDict, StringDict, TadError, _capi
    eng = _FakeEngine(_FakeLib(8191))
    kd, sd = KeyDict(eng, 2), StringDict(eng)                     # the constructors still succeed
    with pytest.raises(TadError) as ei:
        kd.gather(np.zeros(1, np.uint64))
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_DICT_DECODE" in ei.value.message
    with pytest.raises(TadError) as ei:
        sd.decode(np.zeros(1, np.int64))
    assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_DICT_DECODE" in ei.value.message
    with pytest.raises(TadError) as ei:
        sd.take(np.zeros(1, np.int64))
    assert "TAD_FEATURE_DICT_DECODE" in ei.value.message
    for cls, method in ((KeyDict, "gather"), (StringDict, "decode"), (StringDict, "take")):
        assert callable(getattr(cls, method)), method


def test_the_streaming_detector_has_snapshot_and_restore_and_no_host_key_table():
    from theia_amd.stream_detection import StreamingAnomalyDetection
    src = open(os.path.join(ROOT, "theia_amd", "stream_detection.py")).read()
    assert callable(StreamingAnomalyDetection.snapshot) and callable(StreamingAnomalyDetection.restore)
    assert "self._keys" not in src and "_string_at" not in src
    assert ".gather(" in src and ".decode(" in src


def test_go_binding_binds_both_calls_behind_their_guard():
    assert "func hasDictDecode() bool" in GO and "C.tad_features()&C.TAD_FEATURE_DICT_DECODE" in GO
    for name, fn in GO_METHODS.items():
        assert fn in GO, fn
        body = GO[GO.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "C.%s(" % name in body, name
        assert body.index("hasDictDecode()") < body.index("C.%s(" % name), name
    # Gather's pointer array and the columns it names live in C memory: no Go pointer is stored there
    g = GO[GO.index(GO_METHODS["tad_keydict_gather"]):]
    g = g[:g.index("\n}\n")]
    assert "C.calloc(8, C.size_t(unsafe.Sizeof(unsafe.Pointer(nil))))" in g and "defer C.free(unsafe.Pointer(arr))" in g


LAYOUT_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "tad_carve.h"
using namespace tad;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
struct Part { unsigned char *p; size_t bytes; };

// every array inside the block, none touching another: each is filled with its own byte, then all are read back
static void disjoint(unsigned char *base, size_t bytes, const Part *parts, int np) {
  for (int k = 0; k < np; ++k) {
    CHECK(parts[k].p >= base && parts[k].p + parts[k].bytes <= base + bytes);
    CHECK((parts[k].p - base) % 256 == 0);
    memset(parts[k].p, k + 1, parts[k].bytes);
  }
  for (int k = 0; k < np; ++k)
    for (size_t j = 0; j < parts[k].bytes; ++j) CHECK(parts[k].p[j] == (unsigned char)(k + 1));
}

int main() {
  long blocks = 0;
  for (uint64_t n : {1, 2, 31, 32, 33, 255, 256, 257, 1000})
    for (int n_cols : {1, 2, 3, 8})
      for (unsigned mask = 0; mask < (1u << n_cols); mask += (n_cols == 8 ? 37 : 1))
        for (int with_side = 0; with_side < 2; ++with_side)
          for (int host = 0; host < 2; ++host) {
            int asked = 0;
            for (int c = 0; c < n_cols; ++c) asked += (mask >> c) & 1;
            const size_t want = 256 + (host ? up(n * 8) * (1 + asked) + (with_side ? up(n) : 0) : 0);
            Carve m(nullptr);
            const KdGatherWs none = kd_gather_layout(m, n, n_cols, mask, with_side != 0, host != 0);
            CHECK(m.bytes() == want && !m.misaligned() && !none.flags && !none.ids && !none.side);
            unsigned char *raw = static_cast<unsigned char *>(aligned_alloc(256, want + 512));
            memset(raw, 0xEE, want + 512);
            Carve c(raw + 256);
            const KdGatherWs w = kd_gather_layout(c, n, n_cols, mask, with_side != 0, host != 0);
            CHECK(c.bytes() == want && !c.misaligned());
            Part parts[11];
            int np = 0;
            parts[np++] = Part{reinterpret_cast<unsigned char *>(w.flags), 4};
            CHECK((w.ids != nullptr) == (host != 0) && (w.side != nullptr) == (host && with_side));
            if (host) parts[np++] = Part{reinterpret_cast<unsigned char *>(w.ids), (size_t)n * 8};
            for (int i = 0; i < 8; ++i) {
              CHECK((w.col[i] != nullptr) == (host && i < n_cols && ((mask >> i) & 1)));
              if (w.col[i]) parts[np++] = Part{reinterpret_cast<unsigned char *>(w.col[i]), (size_t)n * 8};
            }
            if (w.side) parts[np++] = Part{w.side, (size_t)n};
            disjoint(raw + 256, want, parts, np);
            for (int j = 0; j < 256; ++j) CHECK(raw[j] == 0xEE && raw[256 + want + j] == 0xEE);
            free(raw);
            ++blocks;
          }
  for (uint64_t n : {1, 2, 63, 64, 65, 255, 256, 257, 1000})
    for (int host = 0; host < 2; ++host) {
      const size_t want = 256 + (host ? up(n * 8) : 0) + up(n * 4) + up((n + 1) * 8);
      Carve m(nullptr);
      sd_decode_layout(m, n, host != 0);
      CHECK(m.bytes() == want && !m.misaligned());
      unsigned char *raw = static_cast<unsigned char *>(aligned_alloc(256, want + 512));
      memset(raw, 0xEE, want + 512);
      Carve c(raw + 256);
      const SdDecodeWs w = sd_decode_layout(c, n, host != 0);
      CHECK(c.bytes() == want && !c.misaligned() && (w.codes != nullptr) == (host != 0));
      Part parts[4];
      int np = 0;
      parts[np++] = Part{reinterpret_cast<unsigned char *>(w.flags), 4};
      if (host) parts[np++] = Part{reinterpret_cast<unsigned char *>(w.codes), (size_t)n * 8};
      parts[np++] = Part{reinterpret_cast<unsigned char *>(w.cnt), (size_t)n * 4};
      parts[np++] = Part{reinterpret_cast<unsigned char *>(w.off), (size_t)(n + 1) * 8};
      disjoint(raw + 256, want, parts, np);
      for (int j = 0; j < 256; ++j) CHECK(raw[j] == 0xEE && raw[256 + want + j] == 0xEE);
      free(raw);
      ++blocks;
    }
  printf("blocks %ld\n", blocks);
  return 0;
}
"""


def test_the_two_workspace_layouts_measure_what_they_place(tmp_path):
    src = tmp_path / "decode_layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "decode_layout"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "theia_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "blocks" in r.stdout, r.stdout
