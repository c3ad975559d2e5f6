"""Working size on a CPU-only box (include/slideo_amd.h "Working size"): the header declares the calls, the library exports them
at ABI 7 with an unchanged slideo_config, and slideo_working_size — a pure host function — is the size rule, held here to a
restatement of the rule in Python integers."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_working_size", "slideo_matcher_set_working_size", "slideo_matcher_get_working_size",
         "slideo_group_set_working_size", "slideo_reduce_bgr8"]


def rule(w, h, max_w, max_h):
    """The size rule of the header, in Python's unbounded integers."""
    if w <= max_w and h <= max_h:
        return w, h
    if w * max_h >= h * max_w:                                   # width binds
        return max_w, max(1, (2 * h * max_w + w) // (2 * w))
    return max(1, (2 * w * max_h + h) // (2 * h)), max_h         # height binds


def c_rule(L, w, h, mw, mh):
    dw, dh = C.c_int32(-7), C.c_int32(-7)
    assert L.slideo_working_size(w, h, mw, mh, C.byref(dw), C.byref(dh)) == 0, (w, h, mw, mh)
    return dw.value, dh.value


def test_header_declares_the_working_size_calls():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Working size" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field


def test_rule_on_the_fixed_table(capi):
    L = capi.lib()
    table = {
        (3840, 2160, 1920, 1080): (1920, 1080),                  # the 2x2 fast path
        (4096, 2160, 1920, 1080): (1920, 1013),
        (1920, 1080, 1920, 1080): (1920, 1080),                  # untouched
        (1, 1, 1, 1): (1, 1),
        (1, 1, 1920, 1080): (1, 1),
        (4096, 1, 1920, 1080): (1920, 1),
        (1, 4096, 1920, 1080): (1, 1080),
        (4096, 1, 1, 1): (1, 1),
        (1, 4096, 1, 1): (1, 1),
        (640, 360, 1920, 1080): (640, 360),                      # limits larger than the frame
        (640, 360, 4096, 4096): (640, 360),
        (2560, 1440, 1920, 1080): (1920, 1080),
        (1080, 1920, 1920, 1080): (608, 1080),                   # a portrait frame: the height binds (607.5 rounds up)
    }
    for args, want in table.items():
        assert rule(*args) == want, args
        assert c_rule(L, *args) == want, args


def test_rule_on_a_seeded_sweep(capi):
    L = capi.lib()
    rng = np.random.default_rng(20261016)
    for w, h, mw, mh in rng.integers(1, 4097, (10000, 4)).tolist():
        dw, dh = c_rule(L, w, h, mw, mh)
        assert (dw, dh) == rule(w, h, mw, mh), (w, h, mw, mh)
        assert 1 <= dw <= min(w, mw) and 1 <= dh <= min(h, mh), (w, h, mw, mh, dw, dh)
        fits = w <= mw and h <= mh
        assert ((dw, dh) == (w, h)) == fits, (w, h, mw, mh, dw, dh)


def test_argument_errors(capi):
    L = capi.lib()
    dw, dh = C.c_int32(), C.c_int32()
    for bad in ((0, 1080, 1920, 1080), (1920, 0, 1920, 1080), (1920, 1080, 0, 1080), (1920, 1080, 1920, 0),
                (-1, 1080, 1920, 1080), (1920, 1080, -5, 1080), (1920, 1080, 0, 0)):
        assert L.slideo_working_size(*bad, C.byref(dw), C.byref(dh)) == 1, bad
    assert L.slideo_working_size(1920, 1080, 1280, 720, None, C.byref(dh)) == 1
    assert L.slideo_working_size(1920, 1080, 1280, 720, C.byref(dw), None) == 1
    assert L.slideo_matcher_set_working_size(None, 1920, 1080) == 1
    assert L.slideo_matcher_get_working_size(None, C.byref(dw), C.byref(dh)) == 1
    assert L.slideo_group_set_working_size(None, 1920, 1080) == 1
    assert L.slideo_reduce_bgr8(None, None, 4, 4, 12, 2, 2, None, C.c_int64(12)) == 1


def test_binding_agrees_with_the_c_function(capi):
    L = capi.lib()
    rng = np.random.default_rng(7)
    for w, h, mw, mh in rng.integers(1, 4097, (500, 4)).tolist():
        assert capi.working_size(w, h, mw, mh) == c_rule(L, w, h, mw, mh)
    for bad in ((0, 1, 1, 1), (1, 1, 0, 0)):
        try:
            capi.working_size(*bad)
        except capi.SlideoError as e:
            assert e.code == 1
        else:
            raise AssertionError(bad)


def test_header_declares_every_symbol_the_binding_binds(capi):
    """Every slideo_* name of the binding's export list is declared in the header (the new ones included)."""
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in capi.EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, src), name


def test_video_matcher_takes_a_working_size():
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(working_size=(1920, 1080))._working_size == (1920, 1080)
    assert mt.HipImageVideoMatcher()._working_size is None
