"""Frame mask on a CPU-only box (include/slideo_amd.h "Frame mask"): the header declares the calls and documents their status
codes, the library exports them at the unchanged ABI with ctypes signatures, and the Python, C++ and Rust mirrors carry the option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_matcher_set_frame_mask", "slideo_matcher_frame_mask_info", "slideo_group_set_frame_mask", "slideo_frame_mask_level"]


def _header():
    return open(os.path.join(ROOT, "include", "slideo_amd.h")).read()


def test_header_declares_the_frame_mask_calls():
    src = _header()
    assert "Frame mask" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src                 # additive: the ABI number other tests pin stays


def test_header_documents_semantics_and_status_codes():
    src = _header()
    sec = src[src.index("/* ---- Frame mask"):src.index("/* ---- Changed-frame gate")]
    for needle in ("recalled, unpinned", "runByPixelsMask", "INTER_LINEAR_EXACT", "threshold(254, THRESH_TOZERO)", "BEFORE retainBest",
                   "DETECTION ONLY", "Pages are never masked", "mask_filter_kernel", "all 255", "all 0"):
        assert needle in sec, needle
    # the status codes of the bad arguments, each named where the call is declared
    for needle in ("SLIDEO_ERR_INVALID_ARG", "SLIDEO_ERR_UNSUPPORTED", "SLIDEO_ERR_STATE", "SLIDEO_ERR_CAPACITY", "mask == NULL clears"):
        assert needle in sec, needle
    assert re.search(r"analysed size differs from the mask's fails\s+\*?\s*with SLIDEO_ERR_INVALID_ARG", sec)
    assert re.search(r"SIFT mode refuses a mask with SLIDEO_ERR_UNSUPPORTED", sec)


def test_library_exports_them_with_signatures(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.slideo_matcher_set_frame_mask.argtypes == [vp, vp, i32, i32, i32]
    assert L.slideo_group_set_frame_mask.argtypes == [vp, vp, i32, i32, i32]
    assert L.slideo_matcher_frame_mask_info.argtypes == [vp, vp, vp, vp]
    assert L.slideo_frame_mask_level.argtypes == [vp, i32, vp, i64, vp, vp]


def test_null_handles_and_arguments(capi):
    L = capi.lib()
    mask = np.full((4, 4), 255, np.uint8)
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.slideo_matcher_set_frame_mask(None, mask.ctypes.data_as(C.c_void_p), 4, 4, 4) == 1
    assert L.slideo_group_set_frame_mask(None, mask.ctypes.data_as(C.c_void_p), 4, 4, 4) == 1
    assert L.slideo_matcher_frame_mask_info(None, C.byref(a), C.byref(b), C.byref(c)) == 1
    assert L.slideo_frame_mask_level(None, 0, mask.ctypes.data_as(C.c_void_p), C.c_int64(16), C.byref(a), C.byref(b)) == 1


def test_binding_checks_the_mask_array(capi):
    class Fake(capi._FrameCalls):
        _SETS = "slideo_matcher_"
        _h = None

        def _check(self, rc):
            raise AssertionError("the library must not be reached")
    for bad in (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32), np.zeros(16, np.uint8)):
        with pytest.raises(capi.SlideoError) as e:
            Fake().set_frame_mask(bad)
        assert e.value.code == 1
    for cls in (capi.Matcher, capi.Group):
        assert callable(getattr(cls, "set_frame_mask"))
    assert callable(capi.Matcher.frame_mask_level)


def test_mirrors_carry_the_option():
    from slideo_amd import matching as mt
    mask = np.full((360, 640), 255, np.uint8)
    assert mt.HipImageVideoMatcher(frame_mask=mask)._frame_mask is mask
    assert mt.HipImageVideoMatcher()._frame_mask is None
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert re.search(r"HipImageVideoMatcher&\s+with_frame_mask\(", hpp) and "slideo_group_set_frame_mask(" in hpp
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert "pub fn %s(" % name in ffi, name


def test_docs_name_the_feature():
    ext = open(os.path.join(ROOT, "docs", "EXTENSIONS.md")).read()
    assert "Frame mask" in ext and "mask_filter_kernel" in ext and "masked re-projection" in ext
    assert "frame mask" in open(os.path.join(ROOT, "README.md")).read().lower()
    assert "slideo_matcher_set_frame_mask" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
