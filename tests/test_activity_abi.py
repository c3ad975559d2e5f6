"""Frame activity map on a CPU-only box (include/slideo_amd.h "Frame activity map"): the header declares the calls, the library
exports them at ABI 7 with their ctypes signatures and an unchanged slideo_config, every call refuses a null handle, the Python
methods, learn_frame_mask and the Rust declarations exist; the numpy restatement (tests/activity_ref.py) on hand-computed cases; and
the kernels' per-thread bodies (csrc/activity.hip.h), compiled for the host plain and with -fsanitize=address,undefined as a
stand-alone program over exact-size heap buffers (tools/activity_hostcheck.cpp), equal the restatement bit for bit."""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import activity_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M = r"slideo_matcher\s*\*\s*m"
_GEOM = r"int32_t width,\s*int32_t height"
_LAY = r"const slideo_yuv420_layout\s*\*\s*layout"
CALLS = {
    "slideo_matcher_activity_begin": _M + r",\s*int32_t delta",
    "slideo_matcher_activity_end": _M,
    "slideo_matcher_observe_frames_bgr8": _M + r",\s*int32_t n_frames,\s*const uint8_t\s*\*\s*frames,\s*" + _GEOM + r",\s*int32_t stride_bytes,\s*int64_t frame_stride_bytes",
    "slideo_matcher_observe_frames_yuv420": _M + r",\s*int32_t n_frames,\s*const uint8_t\s*\*\s*frames,\s*" + _GEOM + r",\s*" + _LAY + r",\s*int64_t frame_stride_bytes",
    "slideo_matcher_observe_frames_bgr8_dev": _M + r",\s*int32_t n_frames,\s*const uint8_t\s*\*\s*frames_dev,\s*" + _GEOM +
                                              r",\s*int32_t stride_bytes,\s*int64_t frame_stride_bytes,\s*void\s*\*\s*hip_stream",
    "slideo_matcher_observe_frames_yuv420_dev": _M + r",\s*int32_t n_frames,\s*const uint8_t\s*\*\s*frames_dev,\s*" + _GEOM + r",\s*" + _LAY +
                                                r",\s*int64_t frame_stride_bytes,\s*void\s*\*\s*hip_stream",
    "slideo_matcher_activity_info": _M + r",\s*int32_t\s*\*\s*aw,\s*int32_t\s*\*\s*ah,\s*int32_t\s*\*\s*pairs,\s*int32_t\s*\*\s*delta",
    "slideo_matcher_activity_counts": _M + r",\s*uint32_t\s*\*\s*out,\s*int64_t capacity_elems,\s*int32_t\s*\*\s*aw,\s*int32_t\s*\*\s*ah,\s*int32_t\s*\*\s*pairs",
    "slideo_matcher_activity_mask": _M + r",\s*int32_t max_share_ppm,\s*int32_t grow,\s*uint8_t\s*\*\s*out,\s*int64_t capacity,\s*int32_t\s*\*\s*aw,\s*int32_t\s*\*\s*ah,"
                                         r"\s*int64_t\s*\*\s*n_active,\s*int64_t\s*\*\s*n_masked",
}
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    "slideo_matcher_activity_begin": [vp, i32],
    "slideo_matcher_activity_end": [vp],
    "slideo_matcher_observe_frames_bgr8": [vp, i32, vp, i32, i32, i32, i64],
    "slideo_matcher_observe_frames_yuv420": [vp, i32, vp, i32, i32, vp, i64],
    "slideo_matcher_observe_frames_bgr8_dev": [vp, i32, vp, i32, i32, i32, i64, vp],
    "slideo_matcher_observe_frames_yuv420_dev": [vp, i32, vp, i32, i32, vp, i64, vp],
    "slideo_matcher_activity_info": [vp, vp, vp, vp, vp],
    "slideo_matcher_activity_counts": [vp, vp, i64, vp, vp, vp],
    "slideo_matcher_activity_mask": [vp, i32, i32, vp, i64, vp, vp, vp, vp],
}


def test_header_declares_the_calls_with_their_signatures():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Frame activity map" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in CALLS.items():
        assert re.search(r"\bint32_t\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7_and_refuses_null_handles(capi):
    L = capi.lib()
    for name, argtypes in ARGTYPES.items():
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes == argtypes, name
        # every call: SLIDEO_ERR_INVALID_ARG for a null handle, without a device
        zeros = [None if t is vp else t(0) for t in argtypes]
        assert getattr(L, name)(*zeros) == 1, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field


def test_python_surface_and_rust_declarations(capi):
    for meth in ("activity_begin", "observe_frames", "observe_frames_yuv420", "observe_frames_dev", "observe_frames_yuv420_dev", "activity_info",
                 "activity_counts", "activity_mask", "activity_end"):
        assert callable(getattr(capi.Matcher, meth)), meth
    from slideo_amd import matching as mt
    sig = inspect.signature(mt.learn_frame_mask)
    assert list(sig.parameters) == ["matcher", "frame_batches", "delta", "max_share", "grow"]
    for k in ("delta", "max_share", "grow"):                     # no default is chosen
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is inspect.Parameter.empty
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert re.search(r"pub fn %s\(" % name, ffi), name


def test_learn_frame_mask_runs_begin_observe_mask_end():
    from slideo_amd import matching as mt

    class Fake:
        def __init__(self):
            self.log = []

        def activity_begin(self, delta):
            self.log.append(("begin", delta))

        def observe_frames(self, frames):
            self.log.append(("observe", len(frames)))

        def activity_mask(self, max_share, grow):
            self.log.append(("mask", max_share, grow))
            return "the mask", 3, 5

        def activity_end(self):
            self.log.append(("end",))

    f = Fake()
    assert mt.learn_frame_mask(f, [[0, 0], [0]], delta=24, max_share=0.5, grow=1) == "the mask"
    assert f.log == [("begin", 24), ("observe", 2), ("observe", 1), ("mask", 0.5, 1), ("end",)]

    class Failing(Fake):
        def observe_frames(self, frames):
            raise RuntimeError("boom")

    g = Failing()
    with pytest.raises(RuntimeError):
        mt.learn_frame_mask(g, [[0]], delta=1, max_share=0.1, grow=0)
    assert g.log[-1] == ("end",)                                  # the accumulator is ended on the way out


# ---- the restatement on hand-computed cases ------------------------------------------------------------------------------------

def _hand_frames():
    """2 rows x 3 columns over 4 frames, delta 10.  (0, 0): B 0 -> 10 -> 10 -> 21: SADs 10 (exactly delta: not moved), 0, 11 (delta +
    1: moved).  (1, 0): (0,0,0) -> (4,3,3) -> (8,7,6) -> (8,7,6): SADs 10, 11, 0 over the three channels.  (2, 1): 0 <-> 255 in every
    channel on every frame: SAD 765 three times.  Every other pixel never changes."""
    f = np.full((4, 2, 3, 3), 77, np.uint8)
    f[:, 0, 0] = [[0, 9, 9], [10, 9, 9], [10, 9, 9], [21, 9, 9]]
    f[:, 0, 1] = [[0, 0, 0], [4, 3, 3], [8, 7, 6], [8, 7, 6]]
    f[:, 1, 2] = [[0, 0, 0], [255, 255, 255], [0, 0, 0], [255, 255, 255]]
    return f


def test_restatement_counts_by_hand():
    f = _hand_frames()
    count, pairs = A.counts(f, 10)
    assert pairs == 3 and count.dtype == np.uint32
    assert count.tolist() == [[1, 1, 0], [0, 0, 3]]
    # delta 0: whatever differs moved; delta 765: nothing can (765 > 765 is false)
    assert A.counts(f, 0)[0].tolist() == [[2, 2, 0], [0, 0, 3]]
    assert A.counts(f, 765)[0].tolist() == [[0, 0, 0], [0, 0, 0]]
    assert A.counts(f, 764)[0].tolist() == [[0, 0, 0], [0, 0, 3]]
    # the first frame forms no pair; the last frame of a call pairs with the first frame of the next
    one, p1 = A.counts(f[:1], 10)
    assert p1 == 0 and one.shape == (2, 3) and not one.any()
    acc = A.Accumulator(10).observe(f[:1]).observe(f[1:3]).observe(f[3:])
    assert acc.pairs == 3 and np.array_equal(acc.count, count) and np.array_equal(acc.last, f[3])


def test_restatement_share_is_strict():
    count = np.array([[1, 2, 0]], np.uint32)
    # 1 * 1e6 == 500000 * 2: equality is not active; one ppm less is
    assert A.active(count, 2, 500000).tolist() == [[False, True, False]]
    assert A.active(count, 2, 499999).tolist() == [[True, True, False]]
    assert A.active(count, 2, 1000000).tolist() == [[False, False, False]]          # no count exceeds pairs
    assert A.active(count, 2, 0).tolist() == [[True, True, False]]                  # share 0: every pixel that ever moved
    big = np.array([[2147483647]], np.uint32)                                       # the products need 64 bits
    assert A.active(big, 2147483647, 999999).tolist() == [[True]] and A.active(big, 2147483647, 1000000).tolist() == [[False]]


def test_restatement_grow_by_hand():
    count = np.zeros((4, 5), np.uint32)
    count[1, 3] = 1
    m0, na, nm = A.mask(count, 1, 0, 0)
    assert (na, nm) == (1, 1) and m0[1, 3] == 0 and (m0 == 0).sum() == 1 and set(np.unique(m0)) == {0, 255}
    m1, na, nm = A.mask(count, 1, 0, 1)
    want = np.full((4, 5), 255, np.uint8)
    want[0:3, 2:5] = 0
    assert (na, nm) == (1, 9) and np.array_equal(m1, want)
    count[3, 4] = 1                                               # a corner: the square is clipped
    m1, na, nm = A.mask(count, 1, 0, 1)
    want[2:4, 3:5] = 0
    assert (na, nm) == (2, 11) and np.array_equal(m1, want)
    m64, na, nm = A.mask(count, 1, 0, 64)                         # larger than either side: everything
    assert (na, nm) == (2, 20) and not m64.any()
    none, na, nm = A.mask(count, 1, 1000000, 64)
    assert (na, nm) == (0, 0) and (none == 255).all()
    rng = np.random.default_rng(11)
    c = (rng.random((23, 31)) < 0.02).astype(np.uint32) * 3
    for grow in (0, 1, 2, 7, 64):
        got, want = A.mask(c, 4, 500000, grow), A.mask_by_definition(c, 4, 500000, grow)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], grow


# ---- the kernels' per-thread bodies, compiled for the host -----------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "slideo_amd", "csrc"), os.path.join(ROOT, "tools", "activity_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostchecks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("activity")
    return {"plain": _build(tmp, "hostcheck", []),
            "sanitized": _build(tmp, "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


SIZES = [(640, 360), (349, 347), (402, 300), (403, 33)]             # aw % 4 in {0, 1, 2, 3}


def _host_cases():
    out = []
    for w, h in SIZES:
        pad4 = (3 * w + 3) // 4 * 4 + 4                             # a padded stride of dword-aligned rows: dword loads, a ragged end
        odd = 3 * w + 5 if (3 * w + 5) % 4 else 3 * w + 6           # a padded stride that is no multiple of 4
        out += [(w, h, None, 0, 9, False), (w, h, odd, 1, 2, True), (w, h, None, 2, 1, True), (w, h, pad4, 0, 9, True),
                (w, h, odd, 3, 9, False), (w, h, None, 0, 1, False), (w, h, pad4, 0, 2, False)]
    return out


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: "%dx%d-s%s-o%d-n%d-%s" % (c[0], c[1], c[2], c[3], c[4], "carry" if c[5] else "first"))
def test_host_build_of_the_kernels_equals_the_restatement(hostchecks, tmp_path, case):
    w, h, stride, ofs, n, carry = case
    stride = stride or 3 * w
    delta, ppm, grow = 24, 300000 + 50000 * ofs, (0, 1, 3, 64)[ofs]
    frames = A.moving_frames(n + 1, h, w, w * 7 + h + n)
    prev, frames = frames[0], frames[1:]
    buf = np.random.default_rng(1).integers(0, 256, (n, h, stride), dtype=np.uint8)
    buf[:, :, :w * 3] = frames.reshape(n, h, w * 3)
    acc = A.Accumulator(delta)
    if carry:
        acc.observe(prev[None])
    acc.observe(frames)
    cin, cout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<9i", w, h, stride, n, ofs, delta, int(carry), ppm, grow) + (prev.tobytes() if carry else b"") + buf.tobytes())
    for name, exe in hostchecks.items():
        if os.path.exists(cout):
            os.remove(cout)
        said = subprocess.check_output([exe, cin, cout]).decode()
        if ofs == 0 and stride % 4 == 0:
            assert "in4 1" in said, said                            # the dword path ran
        raw = open(cout, "rb").read()
        px = w * h
        count = np.frombuffer(raw, np.uint32, px).reshape(h, w)
        last = np.frombuffer(raw, np.uint8, px * 3, px * 4).reshape(h, w, 3)
        assert np.array_equal(count, acc.count), (name, int((count != acc.count).sum()))
        assert np.array_equal(last, frames[-1]), name
        if acc.pairs == 0:
            assert len(raw) == px * 7 and not count.any()
            continue
        want, na, nm = A.mask(acc.count, acc.pairs, ppm, grow)
        mask = np.frombuffer(raw, np.uint8, px, px * 7).reshape(h, w)
        tot = np.frombuffer(raw, np.int64, 2, px * 8)
        assert np.array_equal(mask, want), (name, int((mask != want).sum()))
        assert tot.tolist() == [na, nm] and 0 < na < px, (name, tot, na, nm)
