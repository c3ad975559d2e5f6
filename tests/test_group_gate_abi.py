"""The N-device group's changed-frame gate and the frame-primed gate state on a CPU-only box (include/slideo_amd.h "Changed-frame
gate", the group's form): the header declares the eight calls, the library exports them at an unchanged ABI 7, a NULL handle is
SLIDEO_ERR_INVALID_ARG at every entry (no device is needed to say so), the binding carries the methods, and the task's choice of
a gated handle takes a group of several devices.  What the calls compute is tests/test_gpu_group_gate.py's matter."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIME = ["slideo_matcher_gate_reset_from_frame_bgr8", "slideo_matcher_gate_reset_from_frame_yuv420",
         "slideo_matcher_gate_reset_from_frame_bgr8_dev", "slideo_matcher_gate_reset_from_frame_yuv420_dev"]
GROUP = ["slideo_group_gate_reset", "slideo_group_gate_last_small", "slideo_group_match_changed_frames_bgr8",
         "slideo_group_match_changed_frames_yuv420"]
CALLS = PRIME + GROUP


def test_header_declares_the_eight_calls():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "#define SLIDEO_ABI_VERSION 7" in src
    assert "has no gated form" not in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, code), name


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
        assert getattr(L, name).argtypes, name
    assert len(set(capi.EXPORTS)) == len(capi.EXPORTS)
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    for meth in ("gate_reset_from_frame", "gate_reset_from_frame_yuv420", "gate_reset_from_frame_dev", "gate_reset_from_frame_yuv420_dev"):
        assert callable(getattr(capi.Matcher, meth)), meth
    for meth in ("gate_reset", "gate_last_small", "match_changed_frames", "match_changed_frames_yuv420"):
        assert callable(getattr(capi.Group, meth)), meth
        assert callable(getattr(capi.Matcher, meth)), meth


def test_null_handles_are_invalid_arguments(capi):
    L = capi.lib()
    buf = (C.c_uint8 * 64)()
    f32 = (C.c_float * 4)()
    ver = (C.c_uint8 * 64)()
    lay = capi.yuv420_layout("nv12", 4, 4)[0]
    sw, sh = C.c_int32(), C.c_int32()
    i64 = C.c_int64
    assert L.slideo_matcher_gate_reset_from_frame_bgr8(None, buf, 4, 4, 12) == 1
    assert L.slideo_matcher_gate_reset_from_frame_bgr8(None, None, -4, -4, -12) == 1
    assert L.slideo_matcher_gate_reset_from_frame_yuv420(None, buf, 4, 4, C.byref(lay)) == 1
    assert L.slideo_matcher_gate_reset_from_frame_yuv420(None, None, 4, 4, None) == 1
    assert L.slideo_matcher_gate_reset_from_frame_bgr8_dev(None, None, 4, 4, 12, None) == 1
    assert L.slideo_matcher_gate_reset_from_frame_yuv420_dev(None, None, 4, 4, C.byref(lay), None) == 1
    assert L.slideo_group_gate_reset(None, None, 0, 0) == 1
    assert L.slideo_group_gate_reset(None, buf, -1, -1) == 1
    assert L.slideo_group_gate_last_small(None, buf, i64(64), C.byref(sw), C.byref(sh)) == 1
    assert L.slideo_group_match_changed_frames_bgr8(None, 1, buf, 4, 4, 12, i64(48), buf, f32, ver) == 1
    assert L.slideo_group_match_changed_frames_bgr8(None, -1, None, -4, -4, -12, i64(-48), None, None, None) == 1
    assert L.slideo_group_match_changed_frames_yuv420(None, 1, buf, 4, 4, C.byref(lay), i64(24), buf, f32, ver) == 1
    assert L.slideo_group_match_changed_frames_yuv420(None, -1, None, 4, 4, None, i64(24), None, None, None) == 1


class _PairOnly:
    """A handle over two devices without the gated calls."""
    devices = [0, 1]

    def changed_mask(self, frames, prev_small=None):
        pass


class _StubGroup(_PairOnly):
    """A stub group over two devices with the gated calls of its own."""

    def member(self, i):
        raise AssertionError("a group with gated calls of its own is not gated through a member")

    def gate_reset(self, prev_small=None):
        pass

    def match_changed_frames(self, frames):
        pass


def test_the_task_gates_through_a_group_of_several_devices(capi):
    """The binding's own Group over two devices (no handle behind it, no device needed): the task gates through the group itself,
    never through a member.  Before the group had gated calls this gave None."""
    from slideo_amd import matching as mt
    g = capi.Group.__new__(capi.Group)
    g._h, g.devices = None, [0, 1]
    g.member = lambda i: (_ for _ in ()).throw(AssertionError("a group is not gated through a member"))
    assert mt._gated_matcher(g) is g
    stub = _StubGroup()
    assert mt._gated_matcher(stub) is stub
    assert mt._gated_matcher(_PairOnly()) is None                # a handle without the calls: the mask + kept pair remains


def test_mirrors_call_the_groups_gate():
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    for src in (rs, hpp):
        assert "slideo_group_match_changed_frames_bgr8" in src and "slideo_group_gate_reset" in src
        assert "slideo_group_changed_mask_bgr8" in src           # the pair is still there
