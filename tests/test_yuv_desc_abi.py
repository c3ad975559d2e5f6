"""YUV colour description (include/slideo_amd.h "YUV colour description") without a GPU: the exports, the coefficients against the
header's float64 rule, the 16-bit packed layouts, the layout rules of 16-bit containers and the setter's range checks (through
tools/yuv_desc_hostcheck.cpp, a stand-alone program over csrc/frame_settings.h), and the kernel's per-thread arithmetic compiled
for the host — with and without -fsanitize=address,undefined — against tests/yuv_desc_ref.py at the shapes of the GPU test."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import yuv_desc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_yuv_description", "slideo_matcher_yuv_description", "slideo_group_set_yuv_description",
       "slideo_yuv_coefficients", "slideo_yuv420_layout_packed16"]


def test_header_declares_the_calls_and_constants():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    for name, v in (("MATRIX_BT601", 0), ("MATRIX_BT709", 1), ("RANGE_LIMITED", 0), ("RANGE_FULL", 1), ("DEPTH_8", 0), ("DEPTH_10_MSB", 1),
                    ("DEPTH_10_LSB", 2)):
        assert re.search(r"#define SLIDEO_YUV_%s\s+%d\b" % (name, v), h), name
    assert "#define SLIDEO_ABI_VERSION 7" in h
    assert "YUV colour description" in h and "DEPARTURE" in h.split("YUV colour description", 2)[2]


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.Yuv420Layout) == 32 and C.sizeof(capi.Config) == 168


def test_null_handles_and_arguments(capi):
    L = capi.lib()
    v = C.c_int32()
    assert L.slideo_matcher_set_yuv_description(None, 0, 0, 0) == 1
    assert L.slideo_group_set_yuv_description(None, 0, 0, 0) == 1
    assert L.slideo_matcher_yuv_description(None, C.byref(v), C.byref(v), C.byref(v)) == 1
    assert L.slideo_yuv_coefficients(0, 0, None) == 1
    out = (C.c_int32 * 7)()
    for m, r in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert L.slideo_yuv_coefficients(m, r, out) == 1, (m, r)
    with pytest.raises(capi.SlideoError):
        capi.yuv_coefficients("bt2020", "limited")


@pytest.mark.parametrize("matrix,rng", R.PAIRS)
def test_coefficients(capi, matrix, rng):
    got = capi.yuv_coefficients(matrix, rng)
    if (matrix, rng) == (R.BT601, R.LIMITED):
        assert got == (1220542, 2116026, -409993, -852492, 1673527, 16, 20)      # the header's "YUV 4:2:0 frames" literals
    else:
        assert got == R.rule(matrix, rng)
    hdr = open(HDR).read()
    row = r"\s+".join(str(v) for v in got[:6])
    assert re.search(row, hdr), "the header's table lacks %s" % (got[:6],)
    CY, CUB, CUG, CVG, CVR, yofs, shift = got
    assert shift == 20 and yofs == (0 if rng == R.FULL else 16)
    i32 = 2 ** 31
    for c in (CY, CUB, CUG, CVG, CVR):
        assert abs(c) < 2 ** 23 and abs(c) * 255 < i32
    half = 1 << 19
    ymax = (255 - yofs) * CY
    # every sum of the formula at its extremes: u, v in -128..127
    for lo, hi in ((CVR * -128, CVR * 127), (CUB * -128, CUB * 127),
                   (CVG * 127 + CUG * 127, CVG * -128 + CUG * -128)):
        assert -i32 <= half + lo and ymax + half + hi < i32


def test_names_map_to_the_c_values(capi):
    assert capi.yuv_coefficients("bt709", "full") == capi.yuv_coefficients(1, 1)
    assert capi.YUV_MATRICES == {"bt601": 0, "bt709": 1} and capi.YUV_RANGES == {"limited": 0, "full": 1}
    assert capi.YUV_DEPTHS[8] == 0 and capi.YUV_DEPTHS["10_msb"] == 1 and capi.YUV_DEPTHS["10_lsb"] == 2


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_layout_packed16(capi, fmt):
    w, h = 66, 34
    L8, L16 = capi.yuv420_layout_packed(fmt, w, h), capi.yuv420_layout_packed(fmt, w, h, bytes_per_sample=2)
    assert (L16.y_stride, L16.uv_stride, L16.u_offset, L16.v_offset, L16.uv_step) == \
        (2 * L8.y_stride, 2 * L8.uv_stride, 2 * L8.u_offset, 2 * L8.v_offset, L8.uv_step)
    assert L16.y_stride == 2 * w
    if fmt in ("nv12", "nv21"):
        assert L16.uv_step == 2 and L16.uv_stride == 2 * w and abs(L16.u_offset - L16.v_offset) == 2
        assert min(L16.u_offset, L16.v_offset) == 2 * w * h and (L16.u_offset < L16.v_offset) == (fmt == "nv12")
    else:
        assert L16.uv_step == 1 and L16.uv_stride == w
        assert sorted((L16.u_offset, L16.v_offset)) == [2 * w * h, 2 * w * h + w * h // 2] and (L16.u_offset < L16.v_offset) == (fmt == "i420")
    M, fb = capi.yuv420_layout(fmt, w, h, bytes_per_sample=2)
    assert bytes(M) == bytes(L16) and fb == w * h * 3
    out = capi.Yuv420Layout()
    assert capi.lib().slideo_yuv420_layout_packed16(capi.YUV420_FORMATS[fmt], 65, 34, C.byref(out)) == 5      # odd: UNSUPPORTED, as _packed
    assert capi.lib().slideo_yuv420_layout_packed16(7, 64, 34, C.byref(out)) == 1
    assert capi.lib().slideo_yuv420_layout_packed16(0, 64, 34, None) == 1


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(yuv_description=("bt709", "full"))._yuv_description == ("bt709", "full")
    assert mt.HipImageVideoMatcher()._yuv_description is None
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_yuv_description" in hpp and "slideo_group_set_yuv_description" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "yuv_description" in rs and "slideo_group_set_yuv_description" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    hdr = open(HDR).read()
    for name, v in re.findall(r"#define (SLIDEO_YUV_(?:MATRIX|RANGE|DEPTH)_\w+)\s+(\d+)", hdr):
        assert re.search(r"pub const %s: i32 = %s;" % (name, v), ffi), name


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "YUV colour description"), ("README.md", "set_yuv_description"), ("INTEGRATION.md", "slideo_group_set_yuv_description")):
        assert needle in open(os.path.join(ROOT, f)).read(), f


# ---- tools/yuv_desc_hostcheck.cpp ------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "yuv_desc_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_desc"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_desc_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _say(exe, *args):
    code, _, msg = subprocess.check_output([exe] + [str(a) for a in args]).decode().strip().partition(" ")
    return int(code), msg


def test_setter_range_checks(hostcheck):
    for m, r, d in ((0, 0, 0), (1, 1, 2), (1, 0, 1)):
        code, msg = _say(hostcheck, "propose", m, r, d)
        assert code == 0 and tuple(int(x) for x in msg.split()) == R.coefficients(m, r)
    for bad, word in (((2, 0, 0), "matrix"), ((-1, 0, 0), "matrix"), ((0, 2, 0), "range"), ((0, 0, 3), "depth"), ((0, 0, -1), "depth")):
        code, msg = _say(hostcheck, "propose", *bad)
        assert code == 1 and word in msg, (bad, msg)


def test_layout_rules_of_16_bit_containers(hostcheck):
    """validate w h y_stride uv_stride u_offset v_offset uv_step frame_stride bytes_per_sample, at 64x36."""
    w, h = 64, 36
    luma = 2 * w * h

    def v(bps=2, **f):
        a = dict(y_stride=2 * w, uv_stride=2 * w, u_offset=luma, v_offset=luma + 2, uv_step=2, frame_stride=-1)
        a.update(f)
        return _say(hostcheck, "validate", w, h, a["y_stride"], a["uv_stride"], a["u_offset"], a["v_offset"], a["uv_step"], a["frame_stride"], bps)

    assert v() == (0, str(w * h * 3))                                                    # P010, tight: 3 bytes per pixel
    assert v(uv_stride=w, uv_step=1, u_offset=luma, v_offset=luma + w * h // 2) == (0, str(w * h * 3))      # its planar form
    for f, word in ((dict(y_stride=2 * w - 2), "y_stride"), (dict(uv_stride=2 * w - 2), "uv_stride"),
                    (dict(y_stride=2 * w + 1), "even strides"), (dict(uv_stride=2 * w + 1), "even strides"),
                    (dict(u_offset=luma + 1, v_offset=luma + 3), "even offsets"),
                    (dict(v_offset=luma + 1), "even offsets"),
                    (dict(v_offset=luma + 4), "|v_offset - u_offset| == 2"),
                    (dict(u_offset=luma - 2, v_offset=luma), "overlaps"),               # the last luma sample's two bytes
                    (dict(uv_stride=w, uv_step=1, u_offset=luma, v_offset=luma + w * h // 2 - 2), "overlaps"),
                    (dict(frame_stride=w * h * 3 - 2), "frame_stride"),
                    (dict(frame_stride=w * h * 3 + 1), "even frame_stride")):
        code, msg = v(**f)
        assert code == 1 and word in msg, (f, msg)
    # valid for 8-bit samples, not for the matcher's depth: NV12 tight, by bytes
    nv12 = dict(y_stride=w, uv_stride=w, u_offset=w * h, v_offset=w * h + 1)
    assert v(bps=1, **nv12) == (0, str(w * h * 3 // 2))
    code, msg = v(bps=2, **nv12)
    assert code == 1 and "y_stride" in msg and "16-bit" in msg
    # and the 8-bit rules keep their words
    assert "y_stride" in v(bps=1, **dict(nv12, y_stride=w - 2))[1]
    assert "== 1" in v(bps=1, **dict(nv12, v_offset=w * h + 2))[1]
    assert v(bps=2, y_stride=2 * w)[0] == 0 and _say(hostcheck, "validate", w + 1, h, 2 * w + 2, 2 * w + 2, luma, luma + 2, 2, -1, 2)[0] == 5


def _cases(capi):
    """(w, h, fmt, depth, layout name, layout, frame bytes) over the GPU test's matrix."""
    for w, h in R.SIZES:
        for depth in R.DEPTHS:
            for fmt in R.FORMATS:
                for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                    yield w, h, fmt, depth, name, L, fb


def _run_case(exe, tmp, w, h, desc, L, fb, n, ofs, seed):
    frames = np.stack([R.random_frame(w, h, L, fb, desc[2], seed + i) for i in range(n)])
    cin, cout = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<10i3q", w, h, n, desc[0], desc[1], desc[2], L.y_stride, L.uv_stride, L.uv_step, ofs, L.u_offset, L.v_offset, fb))
        f.write(frames.tobytes())
    flags = subprocess.check_output([exe, "convert", cin, cout]).decode()
    got = np.fromfile(cout, np.uint8).reshape(n, h, w, 3)
    for i in range(n):
        want = R.to_bgr(frames[i], w, h, L, desc)
        assert np.array_equal(got[i], want), (w, h, desc, ofs, i, flags, np.argwhere(got[i] != want)[:4])
    return flags


def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(capi, hostcheck, tmp_path):
    """Every case once, the (matrix, range) pair rotating; two frames each; the source at an aligned base."""
    seen = set()
    for k, (w, h, fmt, depth, name, L, fb) in enumerate(_cases(capi)):
        m, r = R.PAIRS[k % 4]
        flags = _run_case(hostcheck, tmp_path, w, h, (m, r, depth), L, fb, 2, 0, k)
        seen.add((depth, flags.strip()))
    for depth in R.DEPTHS:                      # the wide and the fallback paths were both taken, for luma, chroma and the stores
        for word in ("wide_y 0", "wide_y 1", "wide_c 0", "wide_c 1", "out4 0", "out4 1"):
            assert any(d == depth and word in f for d, f in seen), (depth, word)


def test_sanitized_host_build_over_the_whole_matrix(capi, hostcheck_san, tmp_path):
    """All four pairs, and the source's base at 0, 2 and 4 bytes past the alignment: address and undefined-behaviour checks on
    exact-size buffers (a misaligned wide load, a load past the last sample or a store past the image would be reported)."""
    for k, (w, h, fmt, depth, name, L, fb) in enumerate(_cases(capi)):
        for j, (m, r) in enumerate(R.PAIRS):
            if (w, h) not in ((18, 10), (66, 34)) and j != k % 4:
                continue                        # (every pair at two sizes — one tail, one not —, one rotating pair at the others)
            _run_case(hostcheck_san, tmp_path, w, h, (m, r, depth), L, fb, 1, (0, 2, 4, 1)[(k + j) % 4] if depth == R.D8 else (0, 2, 4, 8)[(k + j) % 4], k)
