"""CPU tests of the narrow input columns (tad.h: TAD_FLAG_KEY_U32 / TAD_FLAG_TIME_U32): the header, the ctypes mirror, the
library's feature query (which needs no device) and the Go binding's guard."""
import ctypes
import os
import re

import numpy as np
import pytest
from job_helpers import HEADER, ROOT, header_define

GO = open(os.path.join(ROOT, "go", "tadengine", "tadengine.go")).read()


def test_header_defines_the_flags_the_sentinel_and_the_feature_query():
    assert header_define("TAD_FLAG_KEY_U32") == "2u"
    assert header_define("TAD_FLAG_TIME_U32") == "4u"
    assert header_define("TAD_KEY_SKIP32") == "UINT32_MAX"
    assert header_define("TAD_FEATURE_NARROW_COLUMNS") == "1u"
    assert re.search(r"\bint tad_features\(void\);", HEADER)
    assert header_define("TAD_ABI_VERSION") == "13"     # old callers leave the bits zero: no ABI bump


def test_ctypes_mirror_and_unchanged_struct_sizes():
    from theia_amd import _capi
    assert (_capi.TAD_FLAG_KEY_U32, _capi.TAD_FLAG_TIME_U32, _capi.TAD_KEY_SKIP32) == (2, 4, (1 << 32) - 1)
    assert _capi.TAD_FEATURE_NARROW_COLUMNS == 1
    assert "tad_features" in _capi.SYMBOLS
    # (the flags live in tad_job.flags; no struct grew: the layouts ABI 13 fixed)
    assert ctypes.sizeof(_capi.Columns) == 96 and ctypes.sizeof(_capi.Job) == 136


def test_library_reports_the_narrow_columns_without_a_device():
    from theia_amd import _capi
    lib = _capi.load_library()
    assert hasattr(lib, "tad_features")
    assert lib.tad_features() & _capi.TAD_FEATURE_NARROW_COLUMNS


def test_python_binding_picks_the_narrow_path_by_dtype():
    from theia_amd import _capi
    from theia_amd.engine import _as_column, _narrow_flags, _narrow_of
    lib = _capi.load_library()
    k32, t32, ti32 = np.arange(5, dtype=np.int32), np.arange(5, dtype=np.uint32), np.arange(5, dtype=np.int32)
    assert _narrow_of(k32, "key") and _narrow_of(k32.astype(np.uint32), "key")
    assert _narrow_of(t32, "time") and not _narrow_of(ti32, "time")      # numpy int32 time: sign-extended as before
    assert _narrow_flags(lib, k32, None, t32, None) == _capi.TAD_FLAG_KEY_U32 | _capi.TAD_FLAG_TIME_U32
    assert _narrow_flags(lib, k32, None, ti32, None) == _capi.TAD_FLAG_KEY_U32
    assert _narrow_flags(lib, k32.astype(np.uint64), None, t32, None) == _capi.TAD_FLAG_TIME_U32
    p, n, dev, keep = _as_column(np.array([-1, 3], dtype=np.int32), np.uint64, narrow="key")
    assert n == 2 and not dev and keep.dtype == np.uint32 and int(keep[0]) == _capi.TAD_KEY_SKIP32
    with pytest.raises(Exception):
        _narrow_flags(lib, k32, k32.astype(np.uint64), t32, None)        # one width per column pair
    torch = pytest.importorskip("torch")
    assert _narrow_of(torch.arange(3, dtype=torch.int32), "time") and _narrow_of(torch.arange(3, dtype=torch.int32), "key")
    assert not _narrow_of(torch.arange(3, dtype=torch.float32), "key")


def test_go_binding_asks_the_library_before_setting_either_flag():
    assert "C.tad_features()" in GO
    first = GO.index("C.tad_features()")
    for flag in ("C.TAD_FLAG_KEY_U32", "C.TAD_FLAG_TIME_U32"):
        assert first < GO.index(flag), flag
    for field in ("KeyID32", "KeyID2_32", "FlowEndS32", "FlowStartS32"):
        assert re.search(r"\b%s\s+\[\]uint32" % field, GO), field
