"""Page sets on a CPU-only box: the header declares the calls, the library exports them, and the binding refuses bad arguments
before any device is involved (include/slideo_amd.h "page sets")."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["slideo_matcher_create_page_set", "slideo_matcher_use_page_set", "slideo_matcher_release_page_set",
         "slideo_matcher_page_set_info", "slideo_group_create_page_set", "slideo_group_use_page_set", "slideo_group_release_page_set"]


def test_header_declares_the_page_set_calls():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS


def test_null_handles_are_invalid_arguments(capi):
    L = capi.lib()
    pages = (C.c_int32 * 2)(0, 1)
    out = C.c_int32()
    assert L.slideo_matcher_create_page_set(None, 2, pages, C.byref(out)) == 1
    assert L.slideo_matcher_use_page_set(None, 0) == 1
    assert L.slideo_matcher_release_page_set(None, 1) == 1
    assert L.slideo_matcher_page_set_info(None, 0, None, None, None, None) == 1
    assert L.slideo_group_create_page_set(None, 2, pages, C.byref(out)) == 1
    assert L.slideo_group_use_page_set(None, 0) == 1
    assert L.slideo_group_release_page_set(None, 1) == 1


@pytest.mark.parametrize("cls", ["Matcher", "Group"])
def test_binding_refuses_bad_arguments_before_the_device(capi, cls):
    obj = getattr(capi, cls).__new__(getattr(capi, cls))     # no handle, no device: the binding's own checks come first
    obj._h = C.c_void_p()
    for bad in ([], [1, 1], [-1], [0.5], [3, 2, 3]):
        with pytest.raises(capi.SlideoError) as e:
            obj.create_page_set(bad)
        assert e.value.code == 1, bad
    for bad in (-1, 1.0, "1", True):
        with pytest.raises(capi.SlideoError) as e:
            obj.use_page_set(bad)
        assert e.value.code == 1, bad
    for bad in (0, -3):
        with pytest.raises(capi.SlideoError) as e:
            obj.release_page_set(bad)
        assert e.value.code == 1, bad
    obj._h = None


def test_video_matcher_refuses_foreign_images():
    from slideo_amd import matching as mt
    vm = mt.HipVideoMatcher(matcher=None, images=["a", "b", "c"])
    assert vm._page_indices(["c", "a"]) == [0, 2]
    with pytest.raises(ValueError):
        vm._page_indices(["d"])
    with pytest.raises(ValueError):
        vm._page_indices([])
