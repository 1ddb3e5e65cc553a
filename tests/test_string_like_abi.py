"""CPU tests of the boundary of LIKE matching on the device (include/tad.h: TAD_FEATURE_STRING_LIKE, TAD_LIKE_NOCASE, tad_strdict_like):
the feature bit and the prototype in the header, where the section stands and what it says, the ctypes mirror, the exported symbol,
tad_features() and the NULL-engine refusals without a device, the kernel's source, the Python wrapper against a library without the bit,
the detector's three routes for a pod_label, and the Go binding's guard.  No compute calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from job_helpers import HEADER, ROOT

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
ARGS = ["tad_engine *e", "const tad_strdict *d", "const uint8_t *pattern", "uint64_t pattern_len", "uint32_t flags", "uint8_t *mask", "uint64_t mask_len",
        "tad_mem memory", "uint64_t *n_matched"]


def test_header_defines_the_bit_the_flag_and_the_prototype_and_keeps_the_abi_version():
    assert re.search(r"#define\s+TAD_FEATURE_STRING_LIKE\s+32768u\b", HEADER)
    assert re.search(r"#define\s+TAD_LIKE_NOCASE\s+1u\b", HEADER)
    assert re.search(r"#define\s+TAD_ABI_VERSION\s+13\b", HEADER)
    proto = re.search(r"\b(\w+)\s+tad_strdict_like\s*\(([^;]*?)\)\s*;", CODE, flags=re.S)
    assert proto and proto.group(1) == "int"
    assert [" ".join(a.split()) for a in proto.group(2).split(",")] == ARGS


def test_header_section_stands_between_the_retire_calls_and_the_progress_calls():
    start = HEADER.index("TAD_FEATURE_STRING_LIKE; check tad_features()")
    assert HEADER.index("int tad_keydict_recode(") < start < HEADER.index("#define TAD_FEATURE_STRING_LIKE") < HEADER.index("int tad_strdict_like(") \
        < HEADER.index("int tad_progress(")
    section = " ".join(HEADER[start:HEADER.index("#define TAD_FEATURE_STRING_LIKE")].replace("\n *", " ").split())
    for must in ("makes that byte a literal", "literal backslash", "the empty run included", "%% is %", "exactly one character", "WHOLE value", "anchored at both ends",
                 "match a newline", 'An empty pattern selects "" alone', "escaped ones included", "'A'..'Z' to 'a'..'z' and nothing else", "0x80..0xBF", "one code point",
                 "advances by the same step", "_like_regex", "no Unicode case folding", "U+212A, U+017F, U+0130 and U+0131", "stale length is refused",
                 "never a short write", "pattern_len <= 1024", "*n_matched may be NULL", "other than TAD_LIKE_NOCASE is refused", "An empty dictionary is TAD_OK",
                 "without a device and writes nothing", "LDS", "aligned 16-byte words", "ONE backtrack point", "value length x pattern length", "workspace_limit",
                 "num_values bytes", "The ABI stays 13 and no struct grows", "Lock order: the dictionary, then a job context", "tools/strdict_like_bench.py"):
        assert must in section, must
    # the section quotes no prototype, and every "...; check tad_features()" phrase is unique: the older tests find theirs by the first occurrence
    assert not re.search(r"\bint tad_\w+\(", section)
    for other in re.findall(r"TAD_FEATURE_\w+; check tad_features\(\)", HEADER):
        assert HEADER.count(other) == 1, other
    # the match call's own paragraph points here for the wildcards, and its prototype is what it was
    sd = HEADER[HEADER.index("TAD_FEATURE_STRING_DICT; check tad_features()"):HEADER.index("int tad_strdict_create(")]
    assert "no % / _ wildcards" in " ".join(sd.replace("\n *", " ").split()) and "tad_strdict_like" in sd
    assert "int tad_strdict_match(tad_engine *e, const tad_strdict *d, int32_t op, const uint8_t *pattern, uint64_t pattern_len, uint8_t *mask," in HEADER


def test_ctypes_mirror():
    from theia_amd import _capi
    assert _capi.TAD_FEATURE_STRING_LIKE == 32768 and _capi.TAD_LIKE_NOCASE == 1 and _capi.TAD_ABI_VERSION == 13
    res, argtypes = _capi.SYMBOLS["tad_strdict_like"]
    assert res is ctypes.c_int and len(argtypes) == len(ARGS)
    assert argtypes[3] == ctypes.c_uint64 and argtypes[4] == ctypes.c_uint32 and argtypes[6] == ctypes.c_uint64 and argtypes[7] == ctypes.c_int
    assert argtypes[8] == ctypes.POINTER(ctypes.c_uint64)
    # no existing struct grew
    assert [ctypes.sizeof(s) for s in (_capi.Job, _capi.Columns, _capi.KeyColumns, _capi.StringColumn, _capi.CompactStats, _capi.MergeStats, _capi.StrdictCompactStats)] \
        == [136, 96, 56, 64, 96, 104, 64]


def test_library_exports_the_symbol_and_reports_the_bit_without_a_device():
    from theia_amd import _capi, build
    build.build_library()
    lib = _capi.load_library()
    assert hasattr(lib, "tad_strdict_like")
    f = lib.tad_features()
    assert f & 32768 and f & _capi.TAD_FEATURE_STRING_LIKE
    assert f & 32767 == 32767                                                               # every earlier bit is still set
    assert lib.tad_abi_version() == 13
    # a NULL engine is refused without a device, and nothing is written
    inv = _capi.TAD_ERR_INVALID_ARGUMENT
    mask = np.full(8, 0x5A, dtype=np.uint8)
    n = ctypes.c_uint64(77)
    pat = (ctypes.c_ubyte * 3)(*b"%a_")
    for mem in (_capi.TAD_MEM_HOST, _capi.TAD_MEM_DEVICE):
        for flags in (0, _capi.TAD_LIKE_NOCASE, 6):
            assert lib.tad_strdict_like(None, None, ctypes.cast(pat, ctypes.c_void_p), 3, flags, mask.ctypes.data, 8, mem, ctypes.byref(n)) == inv
    assert lib.tad_strdict_like(None, None, None, 0, 0, None, 0, _capi.TAD_MEM_HOST, None) == inv
    assert (mask == 0x5A).all() and n.value == 77
    assert b"tad_strdict_like: engine is NULL" in lib.tad_last_error(None)


def test_the_language_lives_in_one_header_and_the_kernel_is_hip_in_the_dictionary_s_unit():
    from theia_amd import build
    csrc = os.path.join(ROOT, "theia_amd", "csrc")
    like = open(os.path.join(csrc, "tad_like.h")).read()
    assert os.path.join(csrc, "tad_like.h") in build.HEADERS
    for name in ("like_compile(", "like_match(", "like_step(", "like_fold(", "kLikeOne", "kLikeAny", "kLikeMaxTokens = 1024", "U+212A", "U+017F", "U+0130", "U+0131",
                 "no Unicode case folding"):
        assert name in like, name
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", like) == ["stdint.h", "hip/hip_runtime.h"]      # (the second under __HIPCC__ only)
    body = like[like.index("TAD_LIKE_FN bool like_match("):]
    assert "like_match(" not in body[30:] and not re.search(r"\basm\b|__asm", like)                       # iterative: it never calls itself
    sd = open(os.path.join(csrc, "tad_strdict.hip")).read()
    kernel = sd[sd.index("void k_sd_like("):sd.index("// tad_strdict_export:")]
    for name in ("__shared__ uint16_t s_tok[kLikeMaxTokens]", "__syncthreads()", "len >= min_len", "const ulonglong2 *w", "like_match(", "block_count_add(s_cnt, n_hit, mine)",
                 "gridDim.x * kSdBlock"):
        assert name in kernel, name
    assert not re.search(r"\w+\[[^\]]*\]\s*=", kernel.replace("s_tok[i] = prog[i]", "").replace("out[c] =", ""))    # no per-lane array is written
    assert "launch_sd_like(" in sd and '#include "tad_like.h"' in open(os.path.join(csrc, "tad_internal.h")).read()
    host = open(os.path.join(csrc, "tad_capi_strdict.cpp")).read()
    body = host[host.index("int tad_strdict_like("):host.index("int tad_strdict_decode(")]
    assert body.index("engine is NULL") < body.index("flags & ~TAD_LIKE_NOCASE") < body.index("lock_guard") < body.index("mask_len != K") < body.index("Lease lease") \
        < body.index("over_limit(") < body.index("like_compile(") < body.index("launch_sd_like(")
    # the match call and its refusal are what they were
    assert "%s: bad arguments (dictionary, op TAD_STR_EQUAL / TAD_STR_CONTAINS_NOCASE, a pattern of at most %u bytes, mask in host or device memory)" in host


class _FakeLib:
    """a library of before the feature: every earlier bit, and not the call"""

    def __init__(self, features):
        self._features = features

    def tad_features(self):
        return self._features

    def tad_strdict_create(self, eng, values, nbytes, out):
        return 0

    def tad_strdict_destroy(self, eng, h):
        pass

    def __getattr__(self, name):
        raise AssertionError("touched %s on a library without TAD_FEATURE_STRING_LIKE" % name)


class _NoFeatures:
    tad_strdict_create = staticmethod(lambda *a: 0)
    tad_strdict_destroy = staticmethod(lambda *a: None)


class _FakeEngine:
    def __init__(self, lib):
        self._lib, self._h = lib, ctypes.c_void_p(1)

    def _check(self, rc):
        assert rc == 0


def test_the_wrapper_raises_cleanly_without_the_feature_bit():
    from theia_amd import StringDict, TadError, _capi
    sd = StringDict(_FakeEngine(_FakeLib(32767)))                  # the constructor still succeeds
    for call in (lambda: sd.like("%a_"), lambda: sd.like(b"x", nocase=True, out="device"), lambda: sd.like("")):
        with pytest.raises(TadError) as ei:
            call()
        assert ei.value.code == _capi.TAD_ERR_INVALID_ARGUMENT and "TAD_FEATURE_STRING_LIKE" in ei.value.message and "tad_strdict_like" in ei.value.message
    old = StringDict.__new__(StringDict)                           # a library of before tad_features
    old._engine, old._h = _FakeEngine(_NoFeatures()), None
    with pytest.raises(TadError) as ei:
        old.like("%")
    assert "TAD_FEATURE_STRING_LIKE" in ei.value.message


def test_the_python_method_has_the_documented_signature():
    from theia_amd import StringDict
    E = inspect.Parameter.empty
    assert [(p.name, p.default) for p in inspect.signature(StringDict.like).parameters.values()] == [("self", E), ("pattern", E), ("nocase", False), ("out", "host")]
    assert "tad_strdict_like" in StringDict.like.__doc__ and "WHOLE" in StringDict.like.__doc__


class _Vocab:
    """records which of the two device calls a pod_label takes; export is the host route's"""

    def __init__(self):
        self.calls = []

    def match(self, op, pattern, out="host"):
        self.calls.append(("match", op, pattern, out))
        return "mask", 0

    def like(self, pattern, nocase=False, out="host"):
        self.calls.append(("like", pattern, nocase, out))
        return "mask", 0

    def values(self):
        self.calls.append(("values",))

        class _V:
            to_pylist = staticmethod(lambda: ['{"app":"café"}', '{"test_key":"v"}'])
        return _V()


def test_the_detector_routes_a_pod_label_three_ways():
    from theia_amd import _capi
    from theia_amd.stream_detection import StreamingAnomalyDetection
    s = StreamingAnomalyDetection.__new__(StreamingAnomalyDetection)
    s.agg_flow, s.pod_ident = "pod", "labels"

    def route(label):
        s._vocab = [_Vocab(), _Vocab()]
        terms = s._terms(label, "", "", "", "")
        assert s._vocab[0].calls == [] and len(terms) == 1 and terms[0][0] == 1
        return s._vocab[1].calls, terms[0][1]

    assert route("web")[0] == [("match", _capi.TAD_STR_CONTAINS_NOCASE, "web", "device")]                          # as before
    assert route("x" * 1024)[0] == [("match", _capi.TAD_STR_CONTAINS_NOCASE, "x" * 1024, "device")]
    for label in ('"test_key":"test_value"', "app%db", "test\\_key", "100%", "_", "x" * 1021 + "_"):
        assert route(label)[0] == [("like", "%" + label + "%", True, "device")], label
    calls, mask = route("x" * 1022 + "_")                                                                              # '%' + label + '%' would pass 1024 bytes
    assert calls == [("values",)] and mask.tolist() == [0, 0]
    calls, mask = route("CAFÉ")                                                                                   # Unicode case folding: the host regex
    assert calls == [("values",)] and mask.tolist() == [1, 0]
    calls, mask = route("café_")
    assert calls == [("values",)] and mask.tolist() == [1, 0]
    doc = " ".join(StreamingAnomalyDetection.__doc__.split())
    assert "StringDict.like(" in doc and "1022" in doc and "non-ASCII" in doc


def test_go_binding_binds_the_call_behind_its_guard():
    assert "func hasStringLike() bool" in GO and "C.tad_features()&C.TAD_FEATURE_STRING_LIKE" in GO
    fn = "func (d *StringDict) Like(pattern []byte, nocase bool) (mask []byte, matched uint64, err error) {"
    assert fn in GO
    body = GO[GO.index(fn):]
    body = body[:body.index("\n}\n")]
    assert "C.tad_strdict_like(" in body and body.index("hasStringLike()") < body.index("C.tad_strdict_like(")
    assert "C.TAD_LIKE_NOCASE" in body and "C.TAD_MEM_HOST" in body
    assert "never compiled" in GO[GO.index("func hasStringLike() bool") - 1500:GO.index("func hasStringLike() bool")]
