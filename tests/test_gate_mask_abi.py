"""Frame mask scope on a CPU-only box (include/slideo_amd.h "Frame mask scope"): the header declares the calls and the two scope
bits at the unchanged ABI, the library exports them with ctypes signatures, slideo_changed_ssd_threshold_n is the smallest changed
SSD under the numpy restatement (tests/gate_mask_ref.py), and the Python, C++ and Rust mirrors carry the option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gate_mask_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slideo_matcher_set_frame_mask_scope": "int32_t", "slideo_matcher_frame_mask_scope": "int32_t",
         "slideo_group_set_frame_mask_scope": "int32_t", "slideo_changed_ssd_threshold_n": "int64_t",
         "slideo_frame_mask_small": "int32_t"}


def _header():
    return open(os.path.join(ROOT, "include", "slideo_amd.h")).read()


def test_header_declares_the_calls_and_the_scope_bits():
    src = _header()
    assert "/* ---- Frame mask scope" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, ret in CALLS.items():
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), code), name
    assert re.search(r"#define\s+SLIDEO_MASK_DETECT\s+1u\b", code) and re.search(r"#define\s+SLIDEO_MASK_GATE\s+2u\b", code)
    assert "#define SLIDEO_ABI_VERSION 7" in src                 # additive: the ABI number other tests pin stays
    sec = src[src.index("/* ---- Frame mask scope"):src.index("/* ---- Changed-frame gate")]
    for needle in ("validity map", "n_valid", "to_small_image", "SLIDEO_ERR_INVALID_ARG", "SLIDEO_ERR_STATE", "SLIDEO_ERR_CAPACITY",
                   "ssd_masked_kernel", "slideo_changed_ssd_threshold_n", "never masked"):
        assert needle in sec, needle
    # the follow-up sentence is struck; the re-projection stays unbuilt, with its reason
    assert "possible follow-up" not in src
    assert "Masked re-projection: not built" in src and "register limit" in src


def test_library_exports_them_with_signatures(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    vp, u32, i32, i64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_int64
    assert L.slideo_matcher_set_frame_mask_scope.argtypes == [vp, u32]
    assert L.slideo_group_set_frame_mask_scope.argtypes == [vp, u32]
    assert L.slideo_matcher_frame_mask_scope.argtypes == [vp, vp]
    assert L.slideo_changed_ssd_threshold_n.argtypes == [C.c_float, i64] and L.slideo_changed_ssd_threshold_n.restype == i64
    assert L.slideo_frame_mask_small.argtypes == [vp, vp, i64, vp, vp, vp]
    assert (capi.MASK_DETECT, capi.MASK_GATE) == (1, 2)


def test_null_handles(capi):
    L = capi.lib()
    scope, a, b, n = C.c_uint32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert L.slideo_matcher_set_frame_mask_scope(None, 3) == 1
    assert L.slideo_group_set_frame_mask_scope(None, 3) == 1
    assert L.slideo_matcher_frame_mask_scope(None, C.byref(scope)) == 1
    assert L.slideo_frame_mask_small(None, None, C.c_int64(0), C.byref(a), C.byref(b), C.byref(n)) == 1


@pytest.mark.parametrize("w,h", [(461, 259), (400, 300), (476, 251), (1, 1)])
def test_threshold_n_is_the_sized_threshold(capi, w, h):
    for s in (0.98, 0.5, 0.999):
        assert capi.changed_ssd_threshold_n(s, w * h) == capi.changed_ssd_threshold(s, w, h)


@pytest.mark.parametrize("n", [1, 7, 114251, 120000])
@pytest.mark.parametrize("s", [0.98, 0.5, 0.999])
def test_threshold_n_is_the_smallest_changed_ssd(capi, n, s):
    t = capi.changed_ssd_threshold_n(s, n)
    assert t == gref.threshold(s, n)
    assert 0 < t <= 255 * 255 * 3 * n
    assert gref.is_changed(t, n, s) and not gref.is_changed(t - 1, n, s)


def test_threshold_n_special_cases(capi):
    L = capi.lib()
    for n in (1, 7, 114251):
        assert not gref.is_changed(255 * 255 * 3 * n, n, -1.0)
        assert capi.changed_ssd_threshold_n(-1.0, n) == gref.INT64_MAX == gref.threshold(-1.0, n)      # even the maximal SSD is unchanged
        assert capi.changed_ssd_threshold_n(0.0, n) == gref.threshold(0.0, n)
        assert gref.is_changed(0, n, 1.5)
        assert capi.changed_ssd_threshold_n(1.5, n) == 0 == gref.threshold(1.5, n)                      # SSD 0 already is changed
    for bad in (0, -5, (1 << 31)):
        assert L.slideo_changed_ssd_threshold_n(C.c_float(0.98), C.c_int64(bad)) == -1
    assert L.slideo_changed_ssd_threshold_n(C.c_float(0.98), C.c_int64((1 << 31) - 1)) > 0
    with pytest.raises(capi.SlideoError):
        capi.changed_ssd_threshold_n(0.98, 0)


def test_mirrors_carry_the_option():
    from slideo_amd import _capi, matching as mt
    mask = np.full((360, 640), 255, np.uint8)
    hm = mt.HipImageVideoMatcher(frame_mask=mask, frame_mask_scope=_capi.MASK_DETECT | _capi.MASK_GATE)
    assert hm._frame_mask is mask and hm._frame_mask_scope == 3
    assert mt.HipImageVideoMatcher()._frame_mask_scope is None
    src = open(os.path.join(ROOT, "slideo_amd", "matching.py")).read()
    assert "m.set_frame_mask_scope(self._frame_mask_scope)" in src
    for cls in (_capi.Matcher, _capi.Group):
        assert callable(cls.set_frame_mask_scope) and callable(cls.frame_mask_small)
        assert isinstance(cls.frame_mask_scope, property)
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert re.search(r"HipImageVideoMatcher&\s+with_frame_mask_scope\(", hpp) and "slideo_group_set_frame_mask_scope(" in hpp
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert "pub fn %s(" % name in ffi, name
    assert "pub const SLIDEO_MASK_DETECT: u32 = 1;" in ffi and "pub const SLIDEO_MASK_GATE: u32 = 2;" in ffi
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    assert "pub frame_mask_scope: u32" in rs and "ffi::slideo_group_set_frame_mask_scope(" in rs


def test_docs_name_the_feature():
    ext = open(os.path.join(ROOT, "docs", "EXTENSIONS.md")).read()
    assert "Frame mask scope" in ext and "ssd_masked_kernel" in ext and "masked re-projection" in ext
    assert "A masked gate SSD" not in ext
    assert "frame mask scope" in open(os.path.join(ROOT, "README.md")).read().lower()
    assert os.path.exists(os.path.join(ROOT, "tools", "gate_mask_rate.py"))
