"""The direct look-up scope on a CPU-only box (include/slideo_amd.h "Direct look-up scope"): the header declares the four calls and the
two constants at the unchanged ABI, the library exports them with ctypes signatures, null handles are refused, the Rust binding and the
Python, C++ and Rust mirrors carry the option, and slideo_direct_ssd_threshold over an n_valid that is no product sw * sh is the
largest SSD whose similarity under the numpy restatement of the host expression (tests/gate_mask_ref.py similarity) is >= t."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import gate_mask_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slideo_matcher_set_direct_scope": "int32_t", "slideo_matcher_direct_scope": "int32_t",
         "slideo_group_set_direct_scope": "int32_t", "slideo_page_small_ssd_valid": "int32_t"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_calls_and_constants():
    src = _read("include", "slideo_amd.h")
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, ret in CALLS.items():
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), code), name
    assert re.search(r"#define\s+SLIDEO_DIRECT_WHOLE\s+0u", code) and re.search(r"#define\s+SLIDEO_DIRECT_VALID\s+1u", code)
    assert "#define SLIDEO_ABI_VERSION 7" in src                 # additive
    sec = src[src.index("/* ---- Direct page look-up"):]
    for needle in ("Direct look-up scope", "n_valid", "slideo_frame_mask_small", "slideo_direct_ssd_threshold(t, n_valid)", "bit for bit",
                   "direct_centre_valid_kernel", "NOT rebuilt", "the fourth set call"):
        assert needle in sec, needle


def test_library_exports_them_with_signatures(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
    assert L.slideo_matcher_set_direct_scope.argtypes == [vp, u32]
    assert L.slideo_group_set_direct_scope.argtypes == [vp, u32]
    assert L.slideo_matcher_direct_scope.argtypes == [vp, vp]
    assert L.slideo_page_small_ssd_valid.argtypes == [vp, vp, i32, i32, i32, vp]
    assert (capi.DIRECT_WHOLE, capi.DIRECT_VALID) == (0, 1)


def test_null_handles(capi):
    L = capi.lib()
    s = C.c_uint32()
    assert L.slideo_matcher_set_direct_scope(None, 1) == 1
    assert L.slideo_matcher_direct_scope(None, C.byref(s)) == 1
    assert L.slideo_group_set_direct_scope(None, 1) == 1
    assert L.slideo_page_small_ssd_valid(None, None, 0, 1, 1, None) == 1


def test_rust_binding_and_mirrors_carry_the_option(capi):
    ffi = _read("crates", "matching-hip", "src", "ffi.rs")
    for name in CALLS:
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert "pub const SLIDEO_DIRECT_WHOLE: u32 = 0;" in ffi and "pub const SLIDEO_DIRECT_VALID: u32 = 1;" in ffi
    lib_rs = _read("crates", "matching-hip", "src", "lib.rs")
    assert "pub direct_scope: u32" in lib_rs
    # the scope is applied before the direct similarity: VALID with a gate mask and t constructs without the refusal
    assert 0 < lib_rs.index("slideo_group_set_direct_scope") < lib_rs.index("slideo_group_set_direct_similarity(h")
    hpp = _read("slideo_amd", "host", "matching.hpp")
    assert "with_direct_scope" in hpp
    assert 0 < hpp.index("slideo_group_set_direct_scope(h->g") < hpp.index("slideo_group_set_direct_similarity(h->g")
    from slideo_amd import matching as mt
    assert "direct_scope" in inspect.signature(mt.HipImageVideoMatcher.__init__).parameters
    py = inspect.getsource(mt.HipImageVideoMatcher.create_video_matcher)
    assert 0 < py.index("set_direct_scope") < py.index("set_direct_similarity")
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_direct_scope") and isinstance(getattr(cls, "direct_scope"), property)
    assert hasattr(capi.Matcher, "page_small_ssd_valid")
    doc = _read("INTEGRATION.md")
    assert "slideo_matcher_set_direct_scope" in doc and "slideo_page_small_ssd_valid" in doc


@pytest.mark.parametrize("n", [1, 7, 95519, 119398])
@pytest.mark.parametrize("t", [0.5, 0.9, 0.98, 1.0])
def test_threshold_over_a_valid_pixel_count(capi, t, n):
    """n_valid is whatever the mask leaves: 95 519 = 23 * 4153 is no sw * sh of a small image."""
    T = capi.direct_ssd_threshold(t, n)
    assert 0 <= T < 255 * 255 * 3 * n
    assert gref.similarity(T, n) >= np.float32(t), (T, gref.similarity(T, n))
    assert not gref.similarity(T + 1, n) >= np.float32(t), (T, gref.similarity(T + 1, n))
