"""Frame pixel format (include/slideo_amd.h "Frame pixel format") without a GPU: the header, the exports at ABI 7, the mirrors, the
pure call slideo_pixel_format_info against the restatement (tests/pixel_format_ref.py), the setter's and the layout rules by their
messages (through tools/pixel_format_hostcheck.cpp, a stand-alone program over csrc/frame_settings.h), and the kernel's per-thread
body compiled for the host — with and without -fsanitize=address,undefined — against the restatement over the matrix of the GPU test."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pixel_format_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_pixel_format", "slideo_matcher_pixel_format", "slideo_group_set_pixel_format", "slideo_pixel_format_info",
       "slideo_pixels_to_bgr8"]
FORMS = {"rgb": "packed3", "bgra": "packed4", "rgba": "packed4", "argb": "packed4", "abgr": "packed4",
         "planar_rgb": "planar", "planar_bgr": "planar", "planar_gbr": "planar"}


def test_header_declares_the_calls_and_constants():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    for v, name in R.C_NAMES.items():
        assert re.search(r"#define %s\s+%d\b" % (name, v), h), name
    assert len(re.findall(r"#define SLIDEO_PIXEL_\w+", h)) == 9
    assert "#define SLIDEO_ABI_VERSION 7" in h
    sec = h.split("---- Frame pixel format", 1)[1].split("/* ----", 1)[0]
    for word in ("THE NAMES KEEP THEIR `bgr8`", "DEPARTURE", "Out of scope", "BGR48", "gbrp10le", "GRAY8", "remultiplied", "Pages",
                 "grey", "3 * height * stride_bytes", "returns, bit for", "closes the first item", "FRAME setting"):
        assert word in sec, word
    # the YUV sampling section's text stays: its out-of-scope list still names the item this section closes
    assert "Out of scope: 4-byte BGRA / RGBA input" in h.split("---- YUV sampling", 1)[1].split("/* ----", 1)[0]


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.Yuv420Layout) == 32 and C.sizeof(capi.Config) == 168


def test_null_handles_and_outputs(capi):
    L = capi.lib()
    v = C.c_int32()
    buf = (C.c_uint8 * 64)()
    assert L.slideo_matcher_set_pixel_format(None, 0) == 1
    assert L.slideo_group_set_pixel_format(None, 0) == 1
    assert L.slideo_matcher_pixel_format(None, C.byref(v)) == 1
    assert L.slideo_pixels_to_bgr8(None, buf, 2, 2, 6, buf, 64) == 1


def test_pixel_format_info_agrees_with_the_restatement(capi):
    L = capi.lib()
    assert capi.PIXEL_FORMATS == R.FORMATS
    for name, v in R.FORMATS.items():
        bpp, planes = C.c_int32(-1), C.c_int32(-1)
        assert L.slideo_pixel_format_info(v, C.byref(bpp), C.byref(planes)) == 0
        assert (bpp.value, planes.value) == R.info(name), name
        assert capi.pixel_format_info(name) == R.info(name) and capi.pixel_format_info(v) == R.info(name)
        assert L.slideo_pixel_format_info(v, None, None) == 0                     # either output may be null
        assert L.slideo_pixel_format_info(v, None, C.byref(planes)) == 0 and planes.value == R.info(name)[1]
    for bad in (-1, 9, 16, 1 << 20):
        bpp, planes = C.c_int32(-1), C.c_int32(-1)
        assert L.slideo_pixel_format_info(bad, C.byref(bpp), C.byref(planes)) == 1
        assert (bpp.value, planes.value) == (-1, -1)
    with pytest.raises(capi.SlideoError):
        capi.pixel_format_value("grey")


def test_enum_setting_still_has_its_nine_names():
    src = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    body = re.search(r"enum Setting \{(.*?)\};", src, re.S).group(1)
    names = [n.strip() for n in body.replace("\n", " ").split(",")]
    assert names == ["SET_WORKING_SIZE", "SET_FRAME_REGION", "SET_FRAME_MASK", "SET_FRAME_MASK_SCOPE", "SET_DIRECT_SIMILARITY", "SET_DIRECT_SCOPE",
                     "SET_YUV_DESCRIPTION", "SET_GATE_REFERENCE", "N_SETTINGS"]
    for unit in ("capi_runtime.hip", "capi_group.hip"):
        text = open(os.path.join(ROOT, "slideo_amd", "csrc", unit)).read()
        assert re.search(r"SET_YUV_DESCRIPTION, \[&\]\(const FrameSettings& s\) \{ return propose_pixel_format\(s, format\); \}", text), unit


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(pixel_format="rgba")._pixel_format == "rgba"
    assert mt.HipImageVideoMatcher()._pixel_format is None
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_pixel_format") and hasattr(cls, "pixel_format")
    assert hasattr(capi.Matcher, "pixels_to_bgr")
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_pixel_format" in hpp and "slideo_group_set_pixel_format" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "pub pixel_format: i32" in rs and "slideo_group_set_pixel_format" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    for v, name in R.C_NAMES.items():
        assert re.search(r"pub const %s: i32 = %d;" % (name, v), ffi), name


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## Frame pixel format"), ("README.md", "set_pixel_format"), ("INTEGRATION.md", "slideo_group_set_pixel_format"),
                      ("README.md", "pixel_format.hip.h")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- tools/pixel_format_hostcheck.cpp ---------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pixel_format_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pixel_format"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pixel_format_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _lines(exe, *args):
    out = subprocess.check_output([exe] + [str(a) for a in args]).decode().strip().split("\n")
    return [(int(l.partition(" ")[0]), l.partition(" ")[2]) if not l.startswith("state") else int(l.split()[1]) for l in out]


def test_host_info_and_channels_agree_with_the_restatement(hostcheck):
    for name, v in R.FORMATS.items():
        ok, bpp, planes, b, g, r = (int(x) for x in subprocess.check_output([hostcheck, "info", str(v)]).split())
        assert ok == 1 and (bpp, planes) == R.info(name)
        assert (b, g, r) == tuple(R.ORDER[name].index(c) for c in "BGR"), name
    for bad in (-1, 9):
        assert subprocess.check_output([hostcheck, "info", str(bad)]).split()[0] == b"0"


def test_propose_pixel_format_refusals_leave_the_settings_before(hostcheck):
    for v in range(9):
        assert _lines(hostcheck, "set", v) == [(0, "ok"), v]
    for bad in (9, -1, 16):
        ok, (code, msg), state = _lines(hostcheck, "set", 3, bad)
        assert ok == (0, "ok") and code == 1 and "pixel format" in msg and str(bad) in msg and state == 3
    assert _lines(hostcheck, "set", 6, 9, 0)[-1] == 0                              # and a good value after a refused one takes


def _v(exe, fmt, w, h, stride, fs=-1):
    return _lines(exe, "validate", R.FORMATS[fmt], w, h, stride, fs)[0]


def test_every_layout_rule_by_its_message(hostcheck):
    w, h = 64, 35
    for fmt in R.NON_DEFAULT:
        bpp, planes = R.info(fmt)
        cname = R.C_NAMES[R.FORMATS[fmt]]
        for name, stride in R.layouts(fmt, w, h):
            sp = R.span(fmt, w, h, stride)
            assert _v(hostcheck, fmt, w, h, stride) == (0, str(sp)), (fmt, name)
            assert _v(hostcheck, fmt, w, h, stride, sp)[0] == 0
            code, msg = _v(hostcheck, fmt, w, h, stride, sp - 1)
            assert code == 1 and "frame_stride" in msg and cname in msg, (fmt, msg)
        code, msg = _v(hostcheck, fmt, w, h, bpp * w - 1)
        assert code == 1 and "stride_bytes %d" % (bpp * w - 1) in msg and cname in msg, (fmt, msg)
        if planes == 3:
            assert "every plane" in msg
            code, msg = _v(hostcheck, fmt, w, h, w, w * h)                          # a frame stride that covers one plane only
            assert code == 1 and "three planes" in msg and cname in msg
        else:
            assert "%d * width" % bpp in msg
        for bw, bh in ((0, h), (w, 0), (-1, h)):
            code, msg = _v(hostcheck, fmt, bw, bh, 4096)
            assert code == 1 and msg.startswith("bad image geometry"), msg
    # a three-byte stride is refused under a four-byte format; a planar stride passes where a packed one would not
    assert _v(hostcheck, "bgra", w, h, 3 * w)[0] == 1 and _v(hostcheck, "rgb", w, h, 3 * w)[0] == 0
    assert _v(hostcheck, "planar_rgb", w, h, w) == (0, str(3 * w * h))


def test_default_format_message_is_validate_images():
    src = open(os.path.join(ROOT, "slideo_amd", "csrc", "capi_runtime.hip")).read()
    assert ('void validate_image(int w, int h, int stride) {\n    if (w < 1 || h < 1 || stride < w * 3) fail(SLIDEO_ERR_INVALID_ARG, '
            '"bad image geometry w=%d h=%d stride=%d", w, h, stride);\n}') in src


def _cases():
    """(format, w, h, layout name, stride) over the GPU test's matrix."""
    for fmt in R.NON_DEFAULT:
        for w, h in R.sizes():
            for name, stride in R.layouts(fmt, w, h):
                yield fmt, w, h, name, stride


def _run_case(exe, tmp, fmt, w, h, stride, n, ofs, seed, slack=0):
    rng = np.random.default_rng(seed)
    sp = R.span(fmt, w, h, stride)
    fs = sp + slack
    imgs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = [R.pack(imgs[i], fmt, stride, fs if i < n - 1 else sp, seed * 7 + i) for i in range(n)]
    for i in range(n):                                             # (the restatement inverts itself)
        assert np.array_equal(R.to_bgr(frames[i], w, h, stride, fmt), imgs[i])
    cin, cout = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<8iq", w, h, n, R.FORMATS[fmt], stride, ofs, 0, 0, fs))
        f.write(np.concatenate(frames).tobytes())
    flags = subprocess.check_output([exe, "convert", cin, cout]).decode()
    got = np.fromfile(cout, np.uint8).reshape(n, h, w, 3)
    assert np.array_equal(got, imgs), (fmt, w, h, stride, ofs, flags, np.argwhere(got != imgs)[:4])
    return flags


def test_host_build_of_the_kernel_equals_the_restatement(hostcheck, tmp_path):
    """Every case with two frames, the source at an aligned base and the frames a span apart, then 4 bytes more: every wide load
    and every fallback path was taken at least once, under both stores."""
    seen = set()
    for k, (fmt, w, h, name, stride) in enumerate(_cases()):
        for slack in (0, 4):
            flags = _run_case(hostcheck, tmp_path, fmt, w, h, stride, 2, 0, k, slack)
            seen.update((FORMS[fmt], word) for word in re.findall(r"\w+ \d+", flags))
    for form, wides in (("packed3", (0, 4)), ("packed4", (0, 4, 8, 16)), ("planar", (0, 4))):
        for word in ["out4 0", "out4 1"] + ["wide %d" % v for v in wides]:
            assert (form, word) in seen, (form, word)


def test_sanitized_host_build_over_the_whole_matrix(hostcheck_san, tmp_path):
    """The whole matrix with the source's base 0, 1, 2, 4 and 8 bytes past the alignment, rotating, one or two frames: address and
    undefined-behaviour checks on exact-size buffers — a wide load at an address that is not a multiple of its size, a load past
    the last byte of the last frame or a store past the image would be reported.  Every base offset meets every format and every
    layout class."""
    offsets = (0, 1, 2, 4, 8)
    met = set()
    for k, (fmt, w, h, name, stride) in enumerate(_cases()):
        for j in range(2):
            ofs = offsets[(k + 2 * j + k // 6) % 5]
            _run_case(hostcheck_san, tmp_path, fmt, w, h, stride, 1 + (k + j) % 2, ofs, 100 + k)
            met.add((fmt, name, ofs))
    for fmt in R.NON_DEFAULT:
        for name in ("tight", "pitch16", "pitch8", "pitch4", "pitch2", "odd"):
            for ofs in offsets:
                assert (fmt, name, ofs) in met, (fmt, name, ofs)
