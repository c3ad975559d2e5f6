"""Frame region on a CPU-only box (include/slideo_amd.h "Frame region"): the header declares the calls, the library exports them
at ABI 7 with an unchanged slideo_config; slideo_frame_region_from_quad — a pure host function — maps the destination corners onto
the quad, returns the exact crop for an integer rectangle and refuses degenerate quads; and the kernel's per-pixel arithmetic
(csrc/frame_region.hip.h rectify_thread), compiled for the host and run lane by lane over the launch grid, equals the numpy
restatement tests/frame_region_ref.py bit for bit.  (The set-time refusals need a matcher, and a matcher needs a device: they are
in tests/test_gpu_frame_region.py.)"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frame_region_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"slideo_matcher_set_frame_region": r"slideo_matcher\s*\*\s*m,\s*int32_t src_w,\s*int32_t src_h,\s*const double\s*\*\s*M,\s*int32_t out_w,\s*int32_t out_h",
         "slideo_matcher_frame_region": r"const slideo_matcher\s*\*\s*m,\s*int32_t\s*\*\s*src_w,\s*int32_t\s*\*\s*src_h,\s*double\s*\*\s*M_out,\s*int32_t\s*\*\s*out_w,\s*int32_t\s*\*\s*out_h,\s*int32_t\s*\*\s*is_set",
         "slideo_group_set_frame_region": r"slideo_group\s*\*\s*g,\s*int32_t src_w,\s*int32_t src_h,\s*const double\s*\*\s*M,\s*int32_t out_w,\s*int32_t out_h",
         "slideo_frame_region_from_quad": r"const double\s*\*\s*quad,\s*int32_t out_w,\s*int32_t out_h,\s*double\s*\*\s*M_out",
         "slideo_rectify_bgr8": r"slideo_matcher\s*\*\s*m,\s*const uint8_t\s*\*\s*bgr,\s*int32_t width,\s*int32_t height,\s*int32_t stride_bytes,\s*uint8_t\s*\*\s*out,\s*int64_t out_capacity"}


def test_header_declares_the_calls_with_their_signatures():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Frame region" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in CALLS.items():
        assert re.search(r"\bint32_t\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    # null handles and outputs are argument errors, without a device
    M = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    v = C.c_int32()
    assert L.slideo_matcher_set_frame_region(None, 64, 64, M, 32, 32) == 1
    assert L.slideo_group_set_frame_region(None, 64, 64, M, 32, 32) == 1
    assert L.slideo_matcher_frame_region(None, C.byref(v), C.byref(v), M, C.byref(v), C.byref(v), C.byref(v)) == 1
    assert L.slideo_rectify_bgr8(None, None, 4, 4, 12, None, C.c_int64(12)) == 1
    assert L.slideo_frame_region_from_quad(None, 32, 32, M) == 1


def _apply(M, u, v):
    M = np.asarray(M, np.float64).reshape(9)
    w = M[6] * u + M[7] * v + M[8]
    return (M[0] * u + M[1] * v + M[2]) / w, (M[3] * u + M[4] * v + M[5]) / w


QUADS = [
    ([(30.5, 20.25), (2370.0, 12.5), (2385.75, 1338.0), (15.0, 1330.5)], 2400, 1350, 1920, 1080),      # a keystoned screen
    ([(640.0, 360.0), (1919.0, 360.0), (1919.0, 1079.0), (640.0, 1079.0)], 2560, 1440, 1280, 720),        # a sub-window: the crop
    ([(640.0, 360.0), (1919.0, 360.0), (1919.0, 1079.0), (640.0, 1079.0)], 2560, 1440, 1920, 1080),       # the sub-window, scaled
    ([(-6.3, -4.2), (101.5, 3.0), (99.0, 66.7), (-3.5, 58.1)], 97, 61, 64, 40),                            # partly outside
    ([(80.0, 0.0), (80.0, 119.0), (0.0, 119.0), (0.0, 0.0)], 81, 120, 120, 81),                            # rotated by 90 degrees
    ([(3000.5, 10.0), (4090.0, 900.0), (3500.0, 4000.0), (100.0, 2000.0)], 4096, 4096, 4096, 2),           # extreme sizes
]


@pytest.mark.parametrize("case", QUADS, ids=lambda c: "%dx%d-%dx%d" % c[1:])
def test_from_quad_maps_the_corners_onto_the_quad(capi, case):
    quad, sw, sh, ow, oh = case
    M = capi.frame_region_from_quad(quad, ow, oh)
    assert M.shape == (3, 3) and M[2, 2] == 1.0
    tol = 1e-9 * max(sw, sh)
    for (u, v), (x, y) in zip([(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)], quad):
        gx, gy = _apply(M, float(u), float(v))
        assert abs(gx - x) <= tol and abs(gy - y) <= tol, ((u, v), (gx, gy), (x, y))


def test_from_quad_of_an_integer_rectangle_is_the_exact_crop(capi):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (120, 200, 3), dtype=np.uint8)
    for x0, y0, w, h in ((20, 8, 100, 64), (0, 0, 200, 120), (197, 117, 3, 3), (1, 2, 2, 2), (33, 5, 101, 77)):
        quad = [(x0, y0), (x0 + w - 1, y0), (x0 + w - 1, y0 + h - 1), (x0, y0 + h - 1)]
        M = capi.frame_region_from_quad(quad, w, h)
        assert M.reshape(9).tolist() == [1.0, 0.0, float(x0), 0.0, 1.0, float(y0), 0.0, 0.0, 1.0], (x0, y0, w, h)
        X, Y = R.coords(M, w, h)
        assert not (X & 31).any() and not (Y & 31).any()
        assert np.array_equal(R.rectify(img, M, w, h), img[y0:y0 + h, x0:x0 + w])


def test_from_quad_refuses_degenerate_quads_and_bad_arguments(capi):
    L = capi.lib()
    M = (C.c_double * 9)()

    def rc(quad, ow=64, oh=48):
        q = (C.c_double * 8)(*[c for p in quad for c in p])
        return L.slideo_frame_region_from_quad(q, ow, oh, M)
    good = [(10, 10), (100, 12), (98, 80), (8, 77)]
    assert rc(good) == 0
    assert rc(good[::-1]) == 0                                              # mirrored: the other orientation is a quad too
    assert rc([(0, 0), (10, 10), (20, 20), (30, 30)]) == 1                  # collinear
    assert rc([(0, 0), (50, 0), (100, 0), (50, 40)]) == 1                   # three corners on a line
    assert rc([(10, 10), (10, 10), (98, 80), (8, 77)]) == 1                 # a repeated corner
    assert rc([(0, 0), (100, 0), (30, 20), (0, 100)]) == 1                  # non-convex (a dart)
    assert rc([(0, 0), (100, 100), (100, 0), (0, 100)]) == 1                # self-crossing (a bow tie)
    assert rc([(0, 0), (100, 0), (float("nan"), 80), (0, 80)]) == 1
    assert rc([(0, 0), (100, 0), (float("inf"), 80), (0, 80)]) == 1
    for ow, oh in ((1, 48), (64, 1), (0, 0), (-3, 48), (4097, 48), (64, 4097)):
        assert rc(good, ow, oh) == 1, (ow, oh)
    assert L.slideo_frame_region_from_quad((C.c_double * 8)(), 64, 48, None) == 1
    with pytest.raises(capi.SlideoError) as e:
        capi.frame_region_from_quad([(0, 0), (10, 10), (20, 20), (30, 30)], 64, 48)
    assert e.value.code == 1
    with pytest.raises(capi.SlideoError):
        capi.frame_region_from_quad([(0, 0), (10, 10), (20, 20)], 64, 48)


def test_restatement_on_hand_computed_pixels():
    """The restatement itself, on values worked out by hand: a half-pixel shift averages neighbours with round-half-up, the
    replicate border, and an identity."""
    img = np.zeros((2, 3, 3), np.uint8)
    img[0, :, 0] = [10, 21, 40]; img[1, :, 0] = [100, 101, 102]
    assert np.array_equal(R.rectify(img, [1, 0, 0, 0, 1, 0, 0, 0, 1], 3, 2), img)
    half = R.rectify(img, [1, 0, 0.5, 0, 1, 0, 0, 0, 1], 3, 1)[0, :, 0]
    assert half.tolist() == [16, 31, 40]                                    # (10 + 21) / 2 = 15.5 -> 16, (21 + 40) / 2 = 30.5 -> 31, border
    down = R.rectify(img, [1, 0, 0, 0, 1, 0.25, 0, 0, 1], 1, 2)[:, 0, 0]
    assert down.tolist() == [33, 100]                                       # 10 * 0.75 + 100 * 0.25 = 32.5 -> 33, border
    out = R.rectify(img, [1, 0, -5, 0, 1, 7, 0, 0, 1], 2, 2)
    assert (out[:, :, 0] == 100).all()                                      # far outside: the nearest corner


def test_video_matcher_takes_a_frame_region():
    from slideo_amd import matching as mt
    reg = (2400, 1350, [(30.5, 20.25), (2370.0, 12.5), (2385.75, 1338.0), (15.0, 1330.5)], 1920, 1080)
    assert mt.HipImageVideoMatcher(frame_region=reg)._frame_region == reg
    assert mt.HipImageVideoMatcher()._frame_region is None


# ---- the kernel's arithmetic, compiled for the host ---------------------------------------------------------------------------

def _quad_map(quad, ow, oh):
    A, b = [], []
    for (u, v), (x, y) in zip([(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)], quad):
        A.append([u, v, 1, 0, 0, 0, -x * u, -x * v]); b.append(x)
        A.append([0, 0, 0, u, v, 1, -y * u, -y * v]); b.append(y)
    return np.append(np.linalg.solve(np.array(A, float), np.array(b, float)), 1.0)


# (name, source w x h, stride or None, M, out w x h): the shapes of tests/test_gpu_frame_region.py
HOST_CASES = [
    ("outside", 97, 61, None, _quad_map([(-6.3, -4.2), (101.5, 3.0), (99.0, 66.7), (-3.5, 58.1)], 64, 40), 64, 40),
    ("pitched", 200, 120, 607, _quad_map([(10.2, 8.1), (190.5, 3.3), (195.0, 115.7), (4.5, 110.1)], 133, 77), 133, 77),
    ("low", 300, 40, None, _quad_map([(5.5, 3.2), (290.1, 1.0), (295.0, 36.7), (2.5, 38.1)], 200, 5), 200, 5),
    ("upscale", 64, 64, None, _quad_map([(1.5, 2.2), (61.1, 0.5), (63.0, 62.7), (0.5, 60.1)], 128, 128), 128, 128),
    ("rot90", 80, 120, None, [0, 1, 0, -1, 0, 119, 0, 0, 1], 120, 80),
    ("affine", 80, 120, None, [0.7, 0.2, 3.3, -0.1, 0.9, 5.5, 0, 0, 2.0], 90, 70),
    ("crop", 200, 120, None, [1, 0, 20, 0, 1, 8, 0, 0, 1], 100, 64),
    ("crop-border", 200, 120, 601, [1, 0, -3, 0, 1, -2, 0, 0, 1], 101, 130),
    ("1wide", 1, 50, None, _quad_map([(-1, 0), (1.5, 2), (2, 48), (-1, 49)], 16, 40), 16, 40),
    ("1high", 50, 1, None, _quad_map([(0, -1), (48.5, -2), (49, 2), (1, 1)], 40, 16), 40, 16),
]


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("frame_region") / "hostcheck")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_region_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c[0])
def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(hostcheck, tmp_path, case):
    name, w, h, stride, M, ow, oh = case
    stride = stride or w * 3
    rng = np.random.default_rng(w * 5 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w * 3] = img.reshape(h, w * 3)
    want = R.rectify(img, M, ow, oh)
    M = np.asarray(M, np.float64)
    kinds = [None] if (M[6] != 0 or M[7] != 0) else [None, 0, 1]              # an affine map also through the general instances
    for ofs in (0, 1, 3):                                                    # the source's base at every byte alignment that matters
        for kind in kinds:
            cin, cout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
            with open(cin, "wb") as f:
                f.write(struct.pack("<7i", w, h, stride, ow, oh, 1, ofs) + M.tobytes() + buf.tobytes())
            subprocess.check_call([hostcheck, cin, cout] + ([str(kind)] if kind is not None else []), stdout=subprocess.DEVNULL)
            got = np.fromfile(cout, np.uint8).reshape(oh, ow, 3)
            assert np.array_equal(got, want), (name, ofs, kind, int((got != want).sum()))
