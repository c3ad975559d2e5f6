"""Direct page look-up on a CPU-only box (include/slideo_amd.h "Direct page look-up"): the header declares the calls at the unchanged
ABI, the library exports them with ctypes signatures, the Rust binding declares them, slideo_direct_ssd_threshold is the largest SSD
whose similarity under the numpy restatement of the host expression (tests/gate_mask_ref.py similarity) is >= t, and the Python, C++
and Rust mirrors carry the option."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gate_mask_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slideo_matcher_set_direct_similarity": "int32_t", "slideo_matcher_direct_similarity": "int32_t",
         "slideo_group_set_direct_similarity": "int32_t", "slideo_direct_ssd_threshold": "int64_t", "slideo_page_small_ssd": "int32_t"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_calls():
    src = _read("include", "slideo_amd.h")
    assert "/* ---- Direct page look-up" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, ret in CALLS.items():
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), code), name
    assert "#define SLIDEO_ABI_VERSION 7" in src                 # additive: the ABI number other tests pin stays
    sec = src[src.index("/* ---- Direct page look-up"):]
    for needle in ("eligible pages", "lowest deck page", "inliers 0", "page_idx >= 0 && inliers == 0", "slideo_direct_ssd_threshold",
                   "SLIDEO_ERR_UNSUPPORTED", "SLIDEO_MASK_GATE", "do NOT look up", "page_ssd_kernel", "direct_gate_kernel"):
        assert needle in sec, needle


def test_library_exports_them_with_signatures(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes is not None, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.slideo_matcher_set_direct_similarity.argtypes == [vp, C.c_float]
    assert L.slideo_group_set_direct_similarity.argtypes == [vp, C.c_float]
    assert L.slideo_matcher_direct_similarity.argtypes == [vp, vp]
    assert L.slideo_direct_ssd_threshold.argtypes == [C.c_float, i64] and L.slideo_direct_ssd_threshold.restype == i64
    assert L.slideo_page_small_ssd.argtypes == [vp, vp, i32, i32, i32, vp]


def test_null_handles(capi):
    L = capi.lib()
    t = C.c_float()
    assert L.slideo_matcher_set_direct_similarity(None, 0.5) == 1
    assert L.slideo_matcher_direct_similarity(None, C.byref(t)) == 1
    assert L.slideo_group_set_direct_similarity(None, 0.5) == 1
    assert L.slideo_page_small_ssd(None, None, 0, 1, 1, None) == 1


@pytest.mark.parametrize("n", [1, 1196, 119399])
@pytest.mark.parametrize("t", [0.5, 0.9, 0.98, 1.0])
def test_threshold_is_the_largest_ssd_at_or_above_t(capi, t, n):
    T = capi.direct_ssd_threshold(t, n)
    assert 0 <= T < 255 * 255 * 3 * n
    assert gref.similarity(T, n) >= np.float32(t), (T, gref.similarity(T, n))
    assert not gref.similarity(T + 1, n) >= np.float32(t), (T, gref.similarity(T + 1, n))


def test_threshold_bad_arguments(capi):
    for t, n in ((0.0, 100), (-0.5, 100), (1.5, 100), (float("nan"), 100), (0.9, 0), (0.9, -3), (0.9, 2 ** 31)):
        assert capi.direct_ssd_threshold(t, n) == -1, (t, n)


def test_rust_binding_and_mirrors_carry_the_option():
    ffi = _read("crates", "matching-hip", "src", "ffi.rs")
    for name in CALLS:
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
    assert re.search(r"pub fn slideo_direct_ssd_threshold\(t: f32, n_pixels: i64\) -> i64;", ffi)
    lib_rs = _read("crates", "matching-hip", "src", "lib.rs")
    assert "pub direct_similarity: f32" in lib_rs and "slideo_group_set_direct_similarity" in lib_rs
    hpp = _read("slideo_amd", "host", "matching.hpp")
    assert "with_direct_similarity" in hpp and "slideo_group_set_direct_similarity" in hpp
    from slideo_amd import matching as mt
    import inspect
    assert "direct_similarity" in inspect.signature(mt.HipImageVideoMatcher.__init__).parameters
    for cls in (capi_mod().Matcher, capi_mod().Group):
        assert hasattr(cls, "set_direct_similarity") and hasattr(cls, "direct_similarity")
    assert hasattr(capi_mod().Matcher, "page_small_ssd")
    assert "slideo_matcher_set_direct_similarity" in _read("INTEGRATION.md")


def capi_mod():
    from slideo_amd import _capi
    return _capi
