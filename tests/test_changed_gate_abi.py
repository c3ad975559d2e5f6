"""The changed-frame gate on a CPU-only box (include/slideo_amd.h "Changed-frame gate"): the header declares the calls, the library
exports them at ABI 7 with an unchanged slideo_config, and slideo_changed_ssd_threshold — a pure host function — is held to a
restatement of the mask call's host expression in numpy float32 / float64, in the same order of operations.

A compute entry point needs a matcher handle, and a handle exists only with a device: without one slideo_matcher_create returns
SLIDEO_ERR_NO_DEVICE (so no gated call can be reached), and a NULL handle is SLIDEO_ERR_INVALID_ARG at every entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPUTE = ["slideo_match_changed_frames_bgr8", "slideo_match_changed_frames_yuv420", "slideo_match_changed_frames_bgr8_dev",
           "slideo_match_changed_frames_yuv420_dev", "slideo_match_changed_frames_submit_dev",
           "slideo_match_changed_frames_submit_yuv420_dev", "slideo_match_changed_frames_collect"]
CALLS = ["slideo_matcher_gate_reset", "slideo_matcher_gate_last_small"] + COMPUTE
INT64_MAX = 2 ** 63 - 1
SIZES = [(461, 259), (400, 300), (1, 1)]
THRESHOLDS = [0.98, 0.5, 0.0, 1.0, 1.25]


def similarity(ssd, sw, sh):
    """changed_mask_impl's host expression: sim = 1 - (float)sqrt((double)ssd) / max_error, max_error in float."""
    e = np.sqrt(np.float64(ssd))
    max_error = np.sqrt(np.float32(np.float32(255.0) * np.float32(255.0) * np.float32(3.0)) * np.float32(sw * sh))
    assert max_error.dtype == np.float32
    return np.float32(1.0) - np.float32(e) / max_error


def changed(ssd, sw, sh, thr):
    s = similarity(ssd, sw, sh)
    assert s.dtype == np.float32
    return bool(s < np.float32(thr))


def max_ssd(sw, sh):
    return 255 * 255 * 3 * sw * sh


def test_header_declares_the_gate_calls():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Changed-frame gate" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src), name
    assert re.search(r"\bint64_t\s+slideo_changed_ssd_threshold\s*\(", src)
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS + ["slideo_changed_ssd_threshold"]:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    for meth in ("gate_reset", "gate_last_small", "match_changed_frames", "match_changed_frames_yuv420", "match_changed_frames_dev",
                 "match_changed_frames_yuv420_dev", "submit_changed_dev", "submit_changed_yuv420_dev", "collect_changed"):
        assert callable(getattr(capi.Matcher, meth)), meth


@pytest.mark.parametrize("sw,sh", SIZES)
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_threshold_is_the_first_changed_ssd(capi, sw, sh, thr):
    T = capi.changed_ssd_threshold(thr, sw, sh)
    top = max_ssd(sw, sh)
    assert 0 <= top < 2 ** 62                                    # the full range 0 .. 255^2 * 3 * sw * sh is inside int64
    if T == INT64_MAX:
        assert not changed(top, sw, sh, thr) and not changed(0, sw, sh, thr)
    else:
        assert 0 <= T <= top
        assert changed(T, sw, sh, thr)
        if T > 0:
            assert not changed(T - 1, sw, sh, thr)
    # the device's integer rule against the restatement, over a random sample of SSDs and around T
    rng = np.random.default_rng(20261016 + sw)
    sample = np.concatenate([rng.integers(0, top + 1, 4000), np.unique(np.clip(np.arange(-3, 4) + min(T, top), 0, top)), [0, top]])
    for s in sample.tolist():
        assert changed(s, sw, sh, thr) == (s >= T), (s, T)


@pytest.mark.parametrize("sw,sh", SIZES)
def test_expression_is_monotone_in_the_ssd(sw, sh):
    rng = np.random.default_rng(7 + sw)
    s = np.sort(rng.integers(0, max_ssd(sw, sh) + 1, 20000))
    sims = np.array([similarity(int(v), sw, sh) for v in s], np.float32)
    assert (np.diff(sims) <= 0).all()
    assert similarity(0, sw, sh) == np.float32(1.0)


def test_threshold_fixed_points(capi):
    assert capi.changed_ssd_threshold(1.25, 461, 259) == 0       # every frame is changed, identical ones too
    assert capi.changed_ssd_threshold(1.0, 461, 259) == 1        # any difference
    assert capi.changed_ssd_threshold(1.0, 1, 1) == 1
    assert capi.changed_ssd_threshold(float("nan"), 461, 259) == INT64_MAX
    assert capi.changed_ssd_threshold(-1.0, 461, 259) == INT64_MAX
    L = capi.lib()
    for bad in ((0, 259), (461, 0), (-1, 259), (461, -5), (65536, 65536)):
        assert L.slideo_changed_ssd_threshold(C.c_float(0.98), *bad) == -1, bad
        with pytest.raises(capi.SlideoError) as e:
            capi.changed_ssd_threshold(0.98, *bad)
        assert e.value.code == 1


def test_without_a_device_no_gated_call_is_reachable(capi):
    from conftest import HAS_GPU
    if HAS_GPU:
        m = capi.Matcher()
        m.close()
        return
    with pytest.raises(capi.SlideoError) as e:
        capi.Matcher()
    assert e.value.code == 2                                     # SLIDEO_ERR_NO_DEVICE: there is no handle to gate with


def test_null_handles_are_invalid_arguments(capi):
    L = capi.lib()
    buf = (C.c_uint8 * 64)()
    f32 = (C.c_float * 4)()
    ver = (C.c_uint8 * 64)()
    lay = capi.yuv420_layout("nv12", 4, 4)[0]
    t = C.c_int64()
    sw, sh = C.c_int32(), C.c_int32()
    i64 = C.c_int64
    assert L.slideo_matcher_gate_reset(None, None, 0, 0) == 1
    assert L.slideo_matcher_gate_reset(None, buf, -1, -1) == 1
    assert L.slideo_matcher_gate_last_small(None, buf, i64(64), C.byref(sw), C.byref(sh)) == 1
    assert L.slideo_match_changed_frames_bgr8(None, 1, buf, 4, 4, 12, i64(48), buf, f32, ver) == 1
    assert L.slideo_match_changed_frames_bgr8(None, -1, None, -4, -4, -12, i64(-48), None, None, None) == 1
    assert L.slideo_match_changed_frames_yuv420(None, 1, buf, 4, 4, C.byref(lay), i64(24), buf, f32, ver) == 1
    assert L.slideo_match_changed_frames_yuv420(None, -1, None, 4, 4, None, i64(24), None, None, None) == 1
    assert L.slideo_match_changed_frames_bgr8_dev(None, 1, None, 4, 4, 12, i64(48), buf, f32, ver, None) == 1
    assert L.slideo_match_changed_frames_yuv420_dev(None, 1, None, 4, 4, C.byref(lay), i64(24), buf, f32, ver, None) == 1
    assert L.slideo_match_changed_frames_submit_dev(None, 1, None, 4, 4, 12, i64(48), None, C.byref(t)) == 1
    assert L.slideo_match_changed_frames_submit_dev(None, -1, None, -4, 4, 12, i64(48), None, None) == 1
    assert L.slideo_match_changed_frames_submit_yuv420_dev(None, 1, None, 4, 4, C.byref(lay), i64(24), None, C.byref(t)) == 1
    assert L.slideo_match_changed_frames_collect(None, i64(1), buf, f32, ver) == 1
    assert L.slideo_match_changed_frames_collect(None, i64(-1), None, None, None) == 1


def test_binding_refuses_a_bad_small_image_before_the_device(capi):
    obj = capi.Matcher.__new__(capi.Matcher)                     # no handle, no device: the binding's own check comes first
    obj._h = C.c_void_p()
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(capi.SlideoError) as e:
            obj.gate_reset(bad)
        assert e.value.code == 1
    obj._h = None


def test_rust_shim_declares_the_gate_calls():
    src = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in ("slideo_changed_ssd_threshold", "slideo_matcher_gate_reset", "slideo_match_changed_frames_bgr8",
                 "slideo_match_changed_frames_yuv420"):
        assert re.search(r"pub fn %s\(" % name, src), name
