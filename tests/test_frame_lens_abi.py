"""Frame lens and placement lens on a CPU-only box (include/slideo_amd.h "Frame lens", "Placement lens"): the header declares the
calls, the library exports them at ABI 7 with an unchanged slideo_config, the mirrors and documents name them; null handles are
argument errors that touch nothing; slideo_frame_lens_point equals the numpy restatement tests/frame_lens_ref.py bit for bit; the
kernel's per-pixel arithmetic (csrc/frame_lens.hip.h lens_thread), compiled for the host — plain and with the address and
undefined-behaviour sanitizers, as a stand-alone program on exact-size heap buffers — and run lane by lane over the launch grid,
equals the restatement bit for bit on the GPU tap's shapes; the set-time rules and the rules between lens, region and working size
hold through csrc/frame_settings.h on the host (tools/frame_settings_hostcheck.cpp); slideo_placement_lens equals the restatement of
the same algorithm on exact synthetic correspondences.  (A matcher needs a device: the set calls through the C ABI are in
tests/test_gpu_frame_lens.py.)"""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frame_lens_ref as FL
import placement_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LENS = r"int32_t src_w,\s*int32_t src_h,\s*double cx,\s*double cy,\s*double f,\s*double k1,\s*double k2"
CALLS = {"slideo_matcher_set_frame_lens": r"slideo_matcher\s*\*\s*m,\s*" + _LENS,
         "slideo_matcher_frame_lens": r"const slideo_matcher\s*\*\s*m,\s*int32_t\s*\*\s*src_w,\s*int32_t\s*\*\s*src_h,\s*double\s*\*\s*cx,\s*double\s*\*\s*cy,\s*"
                                      r"double\s*\*\s*f,\s*double\s*\*\s*k1,\s*double\s*\*\s*k2,\s*int32_t\s*\*\s*is_set",
         "slideo_group_set_frame_lens": r"slideo_group\s*\*\s*g,\s*" + _LENS,
         "slideo_frame_lens_point": r"double cx,\s*double cy,\s*double f,\s*double k1,\s*double k2,\s*double u,\s*double v,\s*double\s*\*\s*xd,\s*double\s*\*\s*yd",
         "slideo_undistort_bgr8": r"slideo_matcher\s*\*\s*m,\s*const uint8_t\s*\*\s*bgr,\s*int32_t width,\s*int32_t height,\s*int32_t stride_bytes,\s*"
                                  r"uint8_t\s*\*\s*out,\s*int64_t out_capacity",
         "slideo_placement_lens": r"const uint64_t\s*\*\s*n,\s*const uint64_t\s*\*\s*sfx,\s*const uint64_t\s*\*\s*sfy,\s*const uint64_t\s*\*\s*su,\s*"
                                  r"const uint64_t\s*\*\s*sv,\s*int32_t gw,\s*int32_t gh,\s*int32_t cell,\s*int32_t aw,\s*int32_t ah,\s*int64_t min_count,\s*"
                                  r"double cx,\s*double cy,\s*double f,\s*int32_t order,\s*double trim_px,\s*int32_t rounds,\s*int32_t iters,\s*"
                                  r"double\s*\*\s*k_out2,\s*double\s*\*\s*quad_out8,\s*double\s*\*\s*H_out9,\s*int32_t\s*\*\s*cells_used,\s*double\s*\*\s*rms_px"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_calls_with_their_signatures():
    src = _read("include", "slideo_amd.h")
    assert "---- Frame lens" in src and "---- Placement lens" in src
    assert src.index("---- Match placement map") < src.index("---- Placement lens") < src.index("---- Match shading map")
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in CALLS.items():
        assert re.search(r"\bint32_t\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7_and_null_handles_touch_nothing(capi):
    L = capi.lib()
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field
    d = [C.c_double(7.5) for _ in range(5)]
    i = [C.c_int32(77) for _ in range(3)]
    assert L.slideo_matcher_set_frame_lens(None, 64, 64, 31.5, 31.5, 45.0, -0.1, 0.0) == 1
    assert L.slideo_group_set_frame_lens(None, 64, 64, 31.5, 31.5, 45.0, -0.1, 0.0) == 1
    assert L.slideo_matcher_frame_lens(None, C.byref(i[0]), C.byref(i[1]), *[C.byref(x) for x in d], C.byref(i[2])) == 1
    assert [x.value for x in d] == [7.5] * 5 and [x.value for x in i] == [77] * 3
    out = np.full(12, 9, np.uint8)
    assert L.slideo_undistort_bgr8(None, out.ctypes.data_as(C.c_void_p), 2, 2, 6, out.ctypes.data_as(C.c_void_p), C.c_int64(12)) == 1
    assert (out == 9).all()
    assert L.slideo_frame_lens_point(1.0, 1.0, 2.0, 0.1, 0.0, 3.0, 4.0, None, C.byref(d[0])) == 1 and d[0].value == 7.5
    for bad in ((float("nan"), 1.0, 2.0, 0.1, 0.0, 3.0, 4.0), (1.0, 1.0, 0.0, 0.1, 0.0, 3.0, 4.0), (1.0, 1.0, -2.0, 0.1, 0.0, 3.0, 4.0),
                (1.0, 1.0, 2.0, 0.1, 0.0, float("inf"), 4.0)):
        assert L.slideo_frame_lens_point(*bad, C.byref(d[0]), C.byref(d[1])) == 1 and d[0].value == 7.5 and d[1].value == 7.5, bad


def test_mirrors_and_documents_name_the_calls(capi):
    from slideo_amd import matching as mt
    for name in ("set_frame_lens", "frame_lens", "clear_frame_lens", "undistort", "undistort_pitched"):
        assert hasattr(capi.Matcher, name), name
    assert hasattr(capi.Group, "set_frame_lens") and callable(capi.placement_lens) and callable(capi.frame_lens_point)
    lens = (960, 540, 479.5, 269.5, 550.7, -0.08, 0.0)
    assert mt.HipImageVideoMatcher(frame_lens=lens)._frame_lens == lens
    assert mt.HipImageVideoMatcher()._frame_lens is None
    assert callable(mt.learn_frame_lens_from_matches)
    hpp = _read("slideo_amd", "host", "matching.hpp")
    assert "with_frame_lens" in hpp and "slideo_group_set_frame_lens" in hpp and "placement_lens" in hpp
    ffi = _read("crates", "matching-hip", "src", "ffi.rs")
    for name in CALLS:
        assert "pub fn %s(" % name in ffi, name
    assert "frame_lens" in _read("crates", "matching-hip", "src", "lib.rs")
    ext = _read("docs", "EXTENSIONS.md")
    assert "## Frame lens" in ext and "## Placement lens" in ext
    readme = _read("README.md")
    assert "frame_lens.hip.h" in readme and "slideo_placement_lens" in readme
    assert "FrameLens" in _read("slideo_amd", "csrc", "frame_settings.h")


def test_lens_point_equals_the_restatement_bit_for_bit(capi):
    rng = np.random.default_rng(41)
    n = 4000
    cx, cy = rng.uniform(-50, 2000, n), rng.uniform(-50, 1200, n)
    f = rng.uniform(50, 3000, n)
    k1, k2 = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.2, 0.2, n)
    k2[::3] = 0.0
    u, v = rng.uniform(-200, 4200, n), rng.uniform(-200, 4200, n)
    for i in range(n):
        want = FL.point(cx[i], cy[i], f[i], k1[i], k2[i], u[i], v[i])
        got = capi.frame_lens_point(cx[i], cy[i], f[i], k1[i], k2[i], u[i], v[i])
        assert struct.pack("<2d", *got) == struct.pack("<2d", float(want[0]), float(want[1])), i
        assert capi.frame_lens_point(cx[i], cy[i], f[i], 0.0, 0.0, u[i], v[i]) == (u[i], v[i]), "k = 0 is off: the point itself, exactly"
    assert capi.frame_lens_point(10.0, 20.0, 5.0, -0.3, 0.1, 10.0, 20.0) == (10.0, 20.0)           # the centre stays


def test_restatement_on_hand_computed_values():
    """The restatement itself: f = 10, c = (0, 0), the point (6, 8) has r2 = 1; k1 = -0.25 scales it by 0.75, k2 = 0.5 adds 0.5."""
    assert FL.point(0, 0, 10, -0.25, 0, 6, 8) == (4.5, 6.0)
    assert FL.point(0, 0, 10, -0.25, 0.5, 6, 8) == (7.5, 10.0)
    assert FL.point(1, 2, 10, -0.25, 0, 7, 10) == (5.5, 8.0)
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    assert np.array_equal(FL.undistort(img, (3.0, 2.0, 4.0, 0.0, 0.0)), img)                        # k = 0: the identity
    # a region alone through the lens path with k = 0: the integer crop
    assert np.array_equal(FL.undistort(img, (3.0, 2.0, 4.0, 0.0, 0.0), [1, 0, 2, 0, 1, 1, 0, 0, 1], 4, 3), img[1:4, 2:6])
    assert FL.monotone(-0.3, 0.0, 1.0) and not FL.monotone(-0.34, 0.0, 1.0)
    assert FL.monotone(-0.3, 0.12, 1.0) and not FL.monotone(-1.5, 1.0, 1.0) and FL.monotone(-1.5, 1.0, 0.3)
    assert FL.displacement(100.0, -0.08, 0.0, 1.0) == -8.0


# ---- the kernel's arithmetic, compiled for the host ---------------------------------------------------------------------------

def quad_map(quad, ow, oh):
    A, b = [], []
    for (u, v), (x, y) in zip([(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)], quad):
        A.append([u, v, 1, 0, 0, 0, -x * u, -x * v]); b.append(x)
        A.append([0, 0, 0, u, v, 1, -y * u, -y * v]); b.append(y)
    return np.append(np.linalg.solve(np.array(A, float), np.array(b, float)), 1.0)


def lens_of(w, h, k1, k2=0.0, c=None):
    cx, cy, f = FL.defaults(w, h)
    if c is not None:
        cx, cy = c
    return (cx, cy, f, k1, k2)


# (name, source w x h, stride or None, M or None, out w x h or None, lens): the shapes of tests/test_gpu_frame_lens.py, which
# imports this table
TAP_SHAPES = [
    ("barrel", 97, 61, None, None, None, lens_of(97, 61, -0.2)),
    ("pincushion", 96, 60, 293, None, None, lens_of(96, 60, 0.25)),
    ("k2", 64, 64, None, None, None, lens_of(64, 64, -0.3, 0.12)),
    ("offcentre", 80, 50, None, None, None, lens_of(80, 50, -0.1, 0.0, (20.5, 40.25))),
    ("region", 200, 120, 607, quad_map([(10.2, 8.1), (190.5, 3.3), (195.0, 115.7), (4.5, 110.1)], 133, 77), (133, 77), lens_of(200, 120, -0.15)),
    ("region-crop", 200, 120, None, [1, 0, 20, 0, 1, 8, 0, 0, 1], (100, 64), lens_of(200, 120, -0.15)),
    ("upscale", 64, 64, None, quad_map([(1.5, 2.2), (61.1, 0.5), (63.0, 62.7), (0.5, 60.1)], 128, 128), (128, 128), lens_of(64, 64, 0.2)),
    ("1wide", 1, 50, None, quad_map([(-1, 0), (1.5, 2), (2, 48), (-1, 49)], 16, 40), (16, 40), lens_of(1, 50, -0.1)),
    ("1high", 50, 1, None, quad_map([(0, -1), (48.5, -2), (49, 2), (1, 1)], 40, 16), (40, 16), lens_of(50, 1, -0.1)),
    ("blocks", 600, 338, None, quad_map([(53.1, 35.0), (547.5, 24.1), (562.9, 315.5), (40.0, 303.9)], 480, 270), (480, 270), lens_of(600, 338, -0.08)),
]


def tap_input(shape):
    """-> (img [h, w, 3], buf [h, stride]: the image in rows `stride` apart, the pitch bytes noise, stride)."""
    _, w, h, stride = shape[:4]
    stride = stride or w * 3
    rng = np.random.default_rng(w * 5 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w * 3] = img.reshape(h, w * 3)
    return img, buf, stride


def test_the_tap_shapes_say_what_they_are_there_for():
    """Each shape's reason, on the restatement's own coordinates; every lens passes the setter's reach rule."""
    by = {s[0]: s for s in TAP_SHAPES}
    for name, w, h, _, M, out, lens in TAP_SHAPES:
        ow, oh = out or (w, h)
        assert FL.monotone(lens[3], lens[4], FL.reach(lens, w, h, M, ow, oh)), name
    X, Y = FL.coords(by["pincushion"][6], None, 96, 60)
    assert X.min() < 0 and Y.min() < 0 and (X >> 5).max() >= 95 and (Y >> 5).max() >= 59, "samples outside on all four sides"
    X, Y = FL.coords(by["barrel"][6], None, 97, 61)
    assert X.min() > 0 and (X >> 5).max() < 96, "a barrel lens samples inside"
    k = by["k2"][6]
    Xk, _ = FL.coords(k, None, 64, 64)
    X0, _ = FL.coords(k[:4] + (0.0,), None, 64, 64)
    assert np.abs(Xk - X0).max() >= 32, "the second term moves a corner sample by a pixel or more"
    assert by["barrel"][1] % 4 and by["region"][5][0] % 4, "byte stores on the row tail"
    assert by["blocks"][5][0] > 4 * 64 and by["blocks"][5][1] > 4, "more than one block along x and y"


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def hostcheck(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_lens_" + request.param) / "hostcheck")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call([_cxx(), "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + san + ["-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_lens_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: s[0])
def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(hostcheck, tmp_path, shape):
    name, w, h, _, M, out, lens = shape
    img, buf, stride = tap_input(shape)
    ow, oh = out or (w, h)
    want = FL.undistort(img, lens, M, ow, oh)
    Mb = np.asarray(M if M is not None else np.eye(3).reshape(9), np.float64)
    for ofs in (0, 1, 3):                                                    # the source's base at every byte alignment that matters
        cin, cout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        with open(cin, "wb") as f:
            f.write(struct.pack("<8i", w, h, stride, ow, oh, 1, ofs, int(M is not None)) + Mb.tobytes() + struct.pack("<5d", *lens) + buf.tobytes())
        subprocess.check_call([hostcheck, cin, cout], stdout=subprocess.DEVNULL)
        got = np.fromfile(cout, np.uint8).reshape(oh, ow, 3)
        assert np.array_equal(got, want), (name, ofs, int((got != want).sum()))


def test_set_time_rules_and_the_rules_between_settings_on_the_host(tmp_path):
    """tools/frame_settings_hostcheck.cpp walks the lens's range rules, the off value, the reach rule with and without a region, and
    lens x region x working size in both orders through csrc/frame_settings.h; it asserts against codes written from the header."""
    exe = str(tmp_path / "hostcheck")
    subprocess.check_call([_cxx(), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_settings_hostcheck.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    m = re.search(r"frame lens: (\d+) rule checks", out)
    assert m and int(m.group(1)) >= 30, out


# ---- slideo_placement_lens ------------------------------------------------------------------------------------------------------
AW, AH = 960, 540
CX, CY, F = FL.defaults(AW, AH)
ITERS = 100
HT = P.quad_homography(P.KEYSTONE_QUAD, 2, 2)              # the unit slide onto the placement scene's keystoned quad


def _with_outliers(sm, rng, count, shift_px):
    """-> (the sums with `count` cells' frame x moved by shift_px, those cells [(cy, cx)])."""
    sm = sm.copy()
    ys, xs = np.nonzero(sm[0])
    bad = []
    for j in rng.choice(len(ys), count, replace=False):
        sm[1, ys[j], xs[j]] += sm[0, ys[j], xs[j]] * np.uint64(16 * shift_px)
        bad.append((int(ys[j]), int(xs[j])))
    return sm, bad


@pytest.mark.parametrize("cell", [16, 32, 64])
@pytest.mark.parametrize("k", [(-0.08, 0.0, 1), (0.1, 0.0, 1), (-0.12, 0.03, 2)], ids=["barrel", "pincushion", "k1k2"])
def test_placement_lens_equals_the_restatement(capi, cell, k):
    """Exact synthetic correspondences of a keystone under a lens, with outlier cells 20 px off: the kept set is the restatement's
    (it holds no outlier cell; a trim round may also drop an outlier's neighbours, which the untrimmed first fit pulls), the corners lie within 1e-3 px of its corners (test_placement_abi.py's bound for the quad) and of the truth's, and the radial
    displacement f r (g - 1) at the farthest kept cell lies within 1e-3 px of the restatement's."""
    k1, k2, order = k
    rng = np.random.default_rng(cell + 7)
    sm, bad = _with_outliers(FL.sums_of_lens_homography(HT, (CX, CY, F, k1, k2), AW, AH, cell, (3, 9), rng), rng, 3, 20)
    want = FL.placement_lens(sm, cell, AW, AH, 1, CX, CY, F, order, 2.0, 4, ITERS)
    assert want is not None
    total = int((sm[0] > 0).sum())
    assert not set(want["kept"]) & set(bad) and 4 * len(want["kept"]) >= 3 * total, "the outlier cells are dropped, three quarters of the cells stay"
    kk, quad, H, used, rms = capi.placement_lens(sm, cell, AW, AH, 1, CX, CY, F, order, 2.0, 4, ITERS)
    assert used == len(want["kept"])
    q = np.array(quad)
    assert np.abs(q - want["quad"]).max() < 1e-3, (q, want["quad"])
    assert P.corner_error(q) < 1e-3, "exact data: the truth's corners"
    got_d, want_d = FL.displacement(F, kk[0], kk[1], want["R2"]), FL.displacement(F, want["k"][0], want["k"][1], want["R2"])
    assert abs(got_d - want_d) < 1e-3, (got_d, want_d)
    assert abs(got_d - FL.displacement(F, k1, k2, want["R2"])) < 1e-3, "and the truth's displacement"
    assert abs(rms - want["rms"]) < 1e-3 and (order == 2 or kk[1] == 0.0)
    assert np.abs(H - want["H"]).max() < 1e-3 * max(1.0, np.abs(want["H"]).max())
    # H maps the unit slide to ideal pixels: its corners are the quad
    p = H @ np.array([1.0, 1.0, 1.0])
    assert abs(p[0] / p[2] - quad[2][0]) < 1e-9 and abs(p[1] / p[2] - quad[2][1]) < 1e-9


def test_placement_lens_without_distortion_returns_the_quad_of_placement_quad(capi):
    rng = np.random.default_rng(3)
    sm = P.sums_of_homography(HT, AW, AH, 32, (3, 9), rng)
    kk, quad, _, used, _ = capi.placement_lens(sm, 32, AW, AH, 1, CX, CY, F, 1, 2.0, 4, ITERS)
    q0, _, used0, _ = capi.placement_quad(sm, 32, AW, AH, 1, 2.0, 4)
    assert used == used0
    assert np.abs(np.array(quad) - np.array(q0)).max() < 1e-3
    R2 = FL.placement_lens(sm, 32, AW, AH, 1, CX, CY, F, 1, 2.0, 4, ITERS)["R2"]
    assert abs(FL.displacement(F, kk[0], 0.0, R2)) < 1e-3, kk


def test_placement_lens_refusals(capi):
    L = capi.lib()
    rng = np.random.default_rng(5)
    lens = (CX, CY, F, -0.08, 0.0)
    full = FL.sums_of_lens_homography(HT, lens, AW, AH, 32, 4, rng)
    gh, gw = full.shape[1:]
    k, q, H = (C.c_double * 2)(5, 5), (C.c_double * 8)(*[5] * 8), (C.c_double * 9)(*[5] * 9)
    used, rms = C.c_int32(5), C.c_double(5)

    def rc(sm, cell=32, aw=AW, ah=AH, mc=1, cx=CX, cy=CY, f=F, order=1, trim=2.0, rounds=4, iters=ITERS, gw_=None, gh_=None):
        sm = np.ascontiguousarray(sm, np.uint64)
        a = [sm[i].ctypes.data_as(C.c_void_p) for i in range(5)]
        k[:], q[:], H[:] = [5] * 2, [5] * 8, [5] * 9
        used.value, rms.value = 5, 5
        r = L.slideo_placement_lens(*a, gw_ or sm.shape[2], gh_ or sm.shape[1], cell, aw, ah, C.c_int64(mc), cx, cy, f, order, trim, rounds, iters,
                                    k, q, H, C.byref(used), C.byref(rms))
        if r != 0:
            assert list(k) == [5, 5] and list(q) == [5] * 8 and list(H) == [5] * 9 and used.value == 5 and rms.value == 5, "a refusal writes nothing"
        return r
    assert rc(full) == 0
    for kw in (dict(cell=24), dict(aw=0), dict(ah=4097), dict(mc=0), dict(f=0.0), dict(f=float("nan")), dict(cx=float("inf")), dict(order=0),
               dict(order=3), dict(trim=0.0), dict(rounds=9), dict(iters=0), dict(gw_=gw + 1)):
        assert rc(full, **kw) == 1, kw
    # under-determined: four cells at order 1, five at order 2 (4 + order points are needed)
    ys, xs = np.nonzero(full[0])
    pick = [0, len(ys) // 3, 2 * len(ys) // 3, len(ys) - 1, len(ys) // 2]

    def only(idx):
        sm = np.zeros_like(full)
        for j in idx:
            sm[:, ys[j], xs[j]] = full[:, ys[j], xs[j]]
        return sm
    assert rc(only(pick[:4])) == 1 and FL.placement_lens(only(pick[:4]), 32, AW, AH, 1, CX, CY, F, 1, 2.0, 4, ITERS) is None
    assert rc(only(pick[:5]), order=2) == 1
    assert rc(full, mc=5) == 1, "no cell has five keypoints"
    # sums that hold ONE correspondence per cell of the array (the cell a point is stored in is nothing the fit looks at): the
    # unit-slide points `uv` seen through HT and the lens
    def of_points(uv, lens_):
        sm = np.zeros_like(full)
        for c, (u, v) in enumerate(uv):
            p = HT @ np.array([u, v, 1.0])
            X, Y = FL.point(*lens_, p[0] / p[2], p[1] / p[2])
            assert 0 <= X < AW and 0 <= Y < AH
            sm[:, c // gw, c % gw] = [1, int(round(float(X) * 16)), int(round(float(Y) * 16)), int(round(u * 1048576)), int(round(v * 1048576))]
        return sm
    # collinear: points on one line of the slide determine no homography
    row = of_points([(0.05 + 0.03 * i, 0.5) for i in range(30)], lens)
    assert rc(row) == 1 and FL.placement_lens(row, 32, AW, AH, 1, CX, CY, F, 1, 2.0, 4, ITERS) is None
    # a non-monotone result: data of a lens whose radial map turns back inside the kept cells (the forward model is still a map, and
    # the fit recovers its k1; the setter would refuse it, and so does the learner).  The same points under a mild lens pass
    grid = [((i + 0.5) / 20, (j + 0.5) / 12) for j in range(12) for i in range(20)]
    assert not FL.monotone(-0.6, 0.0, 0.8)
    strong = of_points(grid, (CX, CY, F, -0.6, 0.0))
    assert rc(strong, trim=50.0, rounds=0) == 1 and FL.placement_lens(strong, 32, AW, AH, 1, CX, CY, F, 1, 50.0, 0, ITERS, guard=False) is None
    assert rc(of_points(grid, lens), trim=50.0, rounds=0) == 0 and abs(k[0] + 0.08) < 1e-4
    with pytest.raises(capi.SlideoError) as e:
        capi.placement_lens(row, 32, AW, AH, 1, CX, CY, F, 1, 2.0, 4, ITERS)
    assert e.value.code == 1


# ---- the use ---------------------------------------------------------------------------------------------------------------------------

def test_the_use_on_the_cpu(capi, oracle, synth):
    """The keystone scene bent by k1 = -0.08 (tests/frame_lens_ref.py use_scene: 8 frames, ORB-3000, min_rating 12) through the CPU
    restatement of the pipeline, evidence_ref.votes_of and placement_ref at placement_ref.USE's session (cell 32, min_inliers 12,
    reach 24, min_count 2, trim 3 px, 4 rounds) with nothing set, then matched again under three settings: nothing; the quad of
    slideo_placement_quad alone; the lens and quad of slideo_placement_lens at orders 1 and 2 (frame_region_ref.rectify and
    frame_lens_ref.undistort make the analysed images).  Asserted: the library's fit is the restatement's; the largest corner error
    against the scene's quad and the displacement error at the frame's corner are within frame_lens_ref.USE_BOUNDS, which are twice the
    values measured here rounded up; the learnt lens passes the setter's reach rule beside the learnt quad; no setting loses a page.
    Measured (docs/EXTENSIONS.md "Placement lens"): 8 of 8 frames contribute, 199 cells; pages kept 8 / 8 under every setting; mean
    winning inliers 91.6 with nothing set, 122.0 under the quad alone, 118.4 under lens and quad at order 1, 121.8 at order 2 — the lens
    does NOT raise the inliers over the quad alone on this scene, which is recorded as found and not gated —; order 1: k1 -0.0885 (error
    0.0085), largest corner error 2.82 px, displacement error at the frame corner 4.64 px, 156 cells kept at rms 0.91 px; order 2:
    k (-0.0928, 0.0069), 3.15 px, 3.22 px, 155 cells; slideo_placement_quad's own quad, which lies in the camera's coordinates, is 11.95
    px from the ideal corners with 127 cells kept at rms 1.50 px."""
    import evidence_ref as E
    import frame_region_ref as R
    from conftest import small_cfg
    pages, frames, truth, lens = FL.use_scene(synth)
    U = P.USE
    aw, ah = E.CANVAS_W, E.CANVAS_H
    cx, cy, f = lens[:3]
    cfg = small_cfg(oracle, nfeatures=U["nfeatures"], min_rating=U["min_rating"])
    db = oracle.PageDB(cfg)
    db.add_pages(pages, threads=4)
    assert db.finalize() == 0
    train = db.train()
    tp, pxy = E.deck_of(db, len(pages))
    sizes = {p: (pages[p].shape[1], pages[p].shape[0]) for p in range(len(pages))}
    recs = []
    for fr in frames:
        _, cands = db.match_frame_trace(fr)
        kp, desc = oracle.orb(fr, cfg)
        recs.append(P.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, cands, train))
    sm, through, counted = P.sums(recs, cell=U["cell"], aw=aw, ah=ah, min_inliers=U["min_inliers"], reach=U["reach"], model=0, train_page=tp, page_xy=pxy,
                                  page_sizes=sizes, guard=False)
    print("the use on the CPU: %d of %d frames contribute, %d cells of min_count" % (counted, through, int((sm[0] >= U["min_count"]).sum())))
    assert 2 * counted >= through

    def score(name, imgs):
        v = db.match_frames(imgs, threads=4)
        print("  %-24s pages kept %d of %d (right %d), mean winning inliers %.1f" % (name, int((v["page_idx"] >= 0).sum()), len(v), int((v["page_idx"] == truth).sum()),
                                                                                    v["inliers"].mean()))
        return int((v["page_idx"] >= 0).sum())
    kept0 = score("nothing set", frames)
    q0, _, used0, rms0 = capi.placement_quad(sm, U["cell"], aw, ah, U["min_count"], U["trim"], U["rounds"])
    print("  slideo_placement_quad: %d cells, rms %.2f px, %.2f px from the ideal corners" % (used0, rms0, P.corner_error(q0)))
    ow, oh = FL.out_size_of(q0)
    assert score("quad alone", np.stack([R.rectify(x, quad_map(q0, ow, oh), ow, oh) for x in frames])) >= kept0
    for order in (1, 2):
        want = FL.placement_lens(sm, U["cell"], aw, ah, U["min_count"], cx, cy, f, order, U["trim"], U["rounds"], FL.USE_ITERS, guard=False)
        assert want is not None
        k, quad, _, used, rms = capi.placement_lens(sm, U["cell"], aw, ah, U["min_count"], cx, cy, f, order, U["trim"], U["rounds"], FL.USE_ITERS)
        assert np.abs(np.array(quad) - want["quad"]).max() <= 1e-3 and used == len(want["kept"])
        err, derr = P.corner_error(quad), FL.corner_displacement_error(lens, k, aw, ah)
        print("  order %d: k (%.4f, %.4f), k1 error %.4f, %d cells, rms %.2f px, largest corner error %.2f px, displacement error at the frame corner %.2f px"
              % (order, k[0], k[1], k[0] - FL.USE_K1, used, rms, err, derr))
        B, Mz = FL.USE_BOUNDS[order], FL.USE_MEASURED[order]
        assert B["corner_px"] == math.ceil(2 * Mz["corner_px"]) and B["corner_disp_px"] == math.ceil(2 * Mz["corner_disp_px"])
        assert err <= B["corner_px"] and derr <= B["corner_disp_px"]
        ow, oh = FL.out_size_of(quad)
        M = quad_map(quad, ow, oh)
        learnt = (cx, cy, f, k[0], k[1])
        assert FL.monotone(k[0], k[1], FL.reach(learnt, aw, ah, M, ow, oh)), "the setter takes the learnt lens beside the learnt quad"
        assert score("lens + quad, order %d" % order, np.stack([FL.undistort(x, learnt, M, ow, oh) for x in frames])) >= kept0
