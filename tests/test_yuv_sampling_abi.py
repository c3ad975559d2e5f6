"""YUV sampling (include/slideo_amd.h "YUV sampling") without a GPU: the exports, the tight layouts of all twelve formats, the
setter's rules and every layout rule by its message (through tools/yuv_sampling_hostcheck.cpp, a stand-alone program over
csrc/frame_settings.h), the 4:2:0 messages unchanged, and the kernel's per-thread body compiled for the host — with and without
-fsanitize=address,undefined — against tests/yuv_sampling_ref.py over the matrix of the GPU test."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import yuv_desc_ref as D
import yuv_sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_yuv_sampling", "slideo_matcher_yuv_sampling", "slideo_group_set_yuv_sampling", "slideo_yuv_layout_packed"]
ALL_FORMATS = [f for s in R.SAMPLINGS for f in R.FORMATS[s]]


def test_header_declares_the_calls_and_constants():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    for name, v in (("420", 0), ("422", 1), ("444", 2), ("422_PACKED", 3)):
        assert re.search(r"#define SLIDEO_YUV_SAMPLING_%s\s+%d\b" % (name, v), h), name
    for fmt, v in R.FORMAT_VALUES.items():
        fam = "YUV444" if v >= 24 else "YUV422"
        assert re.search(r"#define SLIDEO_%s_%s\s+%d\b" % (fam, fmt.upper(), v), h), fmt
    assert "#define SLIDEO_ABI_VERSION 7" in h
    sec = h.split("---- YUV sampling", 1)[1].split("/* ----", 1)[0]
    for word in ("THE NAMES KEEP THEIR `420`", "DEPARTURE", "Out of scope", "COLOR_YUV2BGR_YUY2", "(u_offset & 1) ^ 1", "uv_step == 4",
                 "BGRA", "Y210", "4:1:1", "siting", "grey"):
        assert word in sec, word


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
    out = capi.Yuv420Layout()
    assert L.slideo_matcher_set_yuv_sampling(None, 0) == 1
    assert L.slideo_group_set_yuv_sampling(None, 0) == 1
    assert L.slideo_matcher_yuv_sampling(None, C.byref(v)) == 1
    assert L.slideo_yuv_layout_packed(16, 64, 36, 1, None) == 1
    for fmt, w, h, b in ((15, 64, 36, 1), (28, 64, 36, 1), (0, 64, 36, 1), (16, 0, 36, 1), (16, 64, 0, 1), (16, 64, 36, 0), (16, 64, 36, 3)):
        assert L.slideo_yuv_layout_packed(fmt, w, h, b, C.byref(out)) == 1, (fmt, w, h, b)


def test_names_map_to_the_c_values(capi):
    assert capi.YUV_SAMPLINGS == {"420": 0, "422": 1, "444": 2, "422_packed": 3}
    assert capi.YUV_FORMATS == R.FORMAT_VALUES
    assert capi.YUV_PACKED_OFFSETS == R.PACKED_OFFSETS
    for s in R.SAMPLINGS:
        for fmt in R.FORMATS[s]:
            assert capi.yuv_format_sampling(fmt) == R.SAMPLING_NAMES[s]
    assert capi.yuv_format_sampling("nv12") == "420"


def _fields(L):
    return (L.y_stride, L.uv_stride, L.u_offset, L.v_offset, L.uv_step)


@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_layout_packed_is_the_restated_tight_layout(capi, fmt):
    s = R.sampling_of(fmt)
    for w, h in ((66, 35), (2, 1), (640, 360)) + (((7, 5),) if s == R.S444 else ()):
        for b in (1, 2):
            if s == R.S422P and b == 2:
                out = capi.Yuv420Layout()
                assert capi.lib().slideo_yuv_layout_packed(R.FORMAT_VALUES[fmt], w, h, 2, C.byref(out)) == 5      # UNSUPPORTED
                continue
            want, fb = R.make_layout(capi, fmt, w, h, b)
            got = capi.yuv_layout_packed(fmt, w, h, b)
            assert _fields(got) == _fields(want), (fmt, w, h, b)
            mine, mfb = capi.yuv_layout(fmt, w, h, bytes_per_sample=b)                  # the Python helper's tight layout is the library's
            assert bytes(mine) == bytes(got) and mfb == fb
            assert fb == w * h * b * (3 if s == R.S444 else 2)
    if s != R.S444:
        out = capi.Yuv420Layout()
        assert capi.lib().slideo_yuv_layout_packed(R.FORMAT_VALUES[fmt], 65, 36, 1, C.byref(out)) == 5           # odd width: UNSUPPORTED


def test_python_layout_helper(capi):
    """The four 4:2:0 names go to yuv420_layout; pitched layouts of the new ones equal the restatement's."""
    for fmt in ("nv12", "nv21", "i420", "yv12"):
        a, b = capi.yuv_layout(fmt, 66, 34, pitch=128, row_align=16), capi.yuv420_layout(fmt, 66, 34, pitch=128, row_align=16)
        assert bytes(a[0]) == bytes(b[0]) and a[1] == b[1]
    for fmt in ALL_FORMATS:
        for b in (1, 2):
            if R.sampling_of(fmt) == R.S422P and b == 2:
                continue
            got = capi.yuv_layout(fmt, 66, 35, pitch=256, row_align=16, bytes_per_sample=b)
            want = R.make_layout(capi, fmt, 66, 35, b, 256, 48)
            assert _fields(got[0]) == _fields(want[0]) and got[1] == want[1], (fmt, b)
    with pytest.raises(ValueError):
        capi.yuv_layout("nv99", 64, 36)


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(yuv_sampling="444")._yuv_sampling == "444"
    assert mt.HipImageVideoMatcher()._yuv_sampling is None
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_yuv_sampling") and hasattr(cls, "yuv_sampling")
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_yuv_sampling" in hpp and "slideo_group_set_yuv_sampling" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "yuv_sampling" in rs and "slideo_group_set_yuv_sampling" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    hdr = open(HDR).read()
    found = re.findall(r"#define (SLIDEO_YUV(?:_SAMPLING|422|444)_\w+)\s+(\d+)", hdr)
    assert len(found) == 16
    for name, v in found:
        assert re.search(r"pub const %s: i32 = %s;" % (name, v), ffi), name


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## YUV sampling"), ("README.md", "set_yuv_sampling"), ("INTEGRATION.md", "slideo_group_set_yuv_sampling"),
                      ("README.md", "yuv_sampling.hip.h")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- tools/yuv_sampling_hostcheck.cpp ---------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "yuv_sampling_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_sampling"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_sampling_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _lines(exe, *args):
    out = subprocess.check_output([exe] + [str(a) for a in args]).decode().strip().split("\n")
    return [(int(l.partition(" ")[0]), l.partition(" ")[2]) if not l.startswith("state") else tuple(int(x) for x in l.split()[1:]) for l in out]


def test_setter_range_checks_and_the_state_before_stays(hostcheck):
    for v in (0, 1, 2, 3):
        assert _lines(hostcheck, "set", "s", v) == [(0, "ok"), (0, 0, 0, v)]
    for bad in (4, -1, 16):
        (code, msg), state = _lines(hostcheck, "set", "s", 2, "s", bad)[1:]
        assert code == 1 and "yuv sampling" in msg and str(bad) in msg and state == (0, 0, 0, 2)
    # the description's setter leaves the sampling alone, and the other way round
    assert _lines(hostcheck, "set", "s", 2, "d", 1, 1, 2)[-1] == (1, 1, 2, 2)
    assert _lines(hostcheck, "set", "d", 1, 0, 1, "s", 1)[-1] == (1, 0, 1, 1)
    # a refused description leaves everything
    assert _lines(hostcheck, "set", "s", 1, "d", 1, 1, 1, "d", 2, 0, 0)[-1] == (1, 1, 1, 1)


def test_packed_with_a_10_bit_depth_is_refused_in_both_orders(hostcheck):
    for depth in (1, 2):
        a = _lines(hostcheck, "set", "d", 1, 0, depth, "s", 3)
        assert a[0] == (0, "ok") and a[1][0] == 5 and "SLIDEO_YUV_SAMPLING_422_PACKED" in a[1][1] and a[2] == (1, 0, depth, 0)
        b = _lines(hostcheck, "set", "s", 3, "d", 1, 0, depth)
        assert b[0] == (0, "ok") and b[1][0] == 5 and "SLIDEO_YUV_SAMPLING_422_PACKED" in b[1][1] and b[2] == (0, 0, 0, 3)
    # packed with another matrix and range at 8 bits is fine; leaving packed first, then the depth, too
    assert _lines(hostcheck, "set", "s", 3, "d", 1, 1, 0)[-1] == (1, 1, 0, 3)
    assert _lines(hostcheck, "set", "s", 3, "s", 1, "d", 0, 0, 2)[-1] == (0, 0, 2, 1)


def _v(exe, sampling, w, h, bps=1, fs=-1, **f):
    return _lines(exe, "validate", sampling, w, h, f["y_stride"], f["uv_stride"], f["u_offset"], f["v_offset"], f["uv_step"], fs, bps)[0]


def _asdict(L):
    return dict(y_stride=L.y_stride, uv_stride=L.uv_stride, u_offset=L.u_offset, v_offset=L.v_offset, uv_step=L.uv_step)


def test_every_new_layout_rule_by_its_message(capi, hostcheck):
    w, h = 64, 35
    # every tight and pitched layout passes, and the span is the frame's furthest byte
    for fmt in ALL_FORMATS:
        s = R.sampling_of(fmt)
        for b in ((1,) if s == R.S422P else (1, 2)):
            L, fb = R.make_layout(capi, fmt, w, h, b)
            assert _v(hostcheck, s, w, h, b, **_asdict(L)) == (0, str(fb)), fmt
            assert _v(hostcheck, s, w, h, b, fs=fb, **_asdict(L))[0] == 0
            code, msg = _v(hostcheck, s, w, h, b, fs=fb - 2, **_asdict(L))
            assert code == 1 and "frame_stride" in msg and R.SAMPLING_NAMES[s][:3] in msg, (fmt, msg)
    # 4:2:2 and 4:4:4, 8-bit and 16-bit
    for s, name, fmts in ((R.S422, "yuv422", ("nv16", "i422")), (R.S444, "yuv444", ("nv24", "i444"))):
        for b in (1, 2):
            nv, _ = R.make_layout(capi, fmts[0], w, h, b)
            pl, _ = R.make_layout(capi, fmts[1], w, h, b)
            nv, pl = _asdict(nv), _asdict(pl)
            luma = w * h * b
            cases = [(dict(nv, uv_step=3), "uv_step 3"), (dict(nv, uv_step=4), "uv_step 4"), (dict(nv, u_offset=-2, v_offset=-2 + b), "negative"),
                     (dict(nv, y_stride=w * b - 2), "y_stride"), (dict(nv, uv_stride=nv["uv_stride"] - 2), "uv_stride"),
                     (dict(pl, uv_stride=pl["uv_stride"] - 2), "uv_stride"),
                     (dict(nv, v_offset=nv["u_offset"] + 2 * b), "|v_offset - u_offset| == %d" % b),
                     (dict(nv, u_offset=luma - 2 * b, v_offset=luma - b), "overlaps"),
                     (dict(pl, v_offset=pl["v_offset"] - 2 * b), "overlaps")]
            if b == 2:
                cases += [(dict(nv, y_stride=2 * w + 1), "even strides"), (dict(nv, u_offset=luma + 1, v_offset=luma + 3), "even offsets")]
            for f, word in cases:
                code, msg = _v(hostcheck, s, w, h, b, **f)
                assert code == 1 and word in msg and msg.startswith(name), (s, b, f, msg)
            if b == 2:
                code, msg = _v(hostcheck, s, w, h, b, fs=luma * 4 + 1, **nv)
                assert code == 1 and "even frame_stride" in msg and msg.startswith(name)
    # a 4:2:0 layout under 4:4:4: the chroma planes are too short — U, of `h` rows now, runs into V
    i420, _ = capi.yuv420_layout("i420", w, 36, pitch=2 * w)
    code, msg = _v(hostcheck, R.S444, w, 36, **_asdict(i420))
    assert code == 1 and "overlaps" in msg and msg.startswith("yuv444") and "36 rows" in msg
    nv12, fb12 = capi.yuv420_layout("nv12", w, 36, pitch=2 * w)
    code, msg = _v(hostcheck, R.S444, w, 36, fs=fb12, **_asdict(nv12))
    assert code == 1 and "frame_stride" in msg and msg.startswith("yuv444")
    # odd sides
    nv16 = _asdict(R.make_layout(capi, "nv16", w + 2, h)[0])
    code, msg = _v(hostcheck, R.S422, w + 1, h, **nv16)
    assert code == 5 and "yuv422" in msg and "even" in msg
    assert _v(hostcheck, R.S444, w + 1, h, **_asdict(R.make_layout(capi, "nv24", w + 1, h)[0]))[0] == 0
    # packed
    yuy2 = _asdict(R.make_layout(capi, "yuy2", w, h)[0])
    for f, word in ((dict(yuy2, uv_step=2), "uv_step 2 is not 4"), (dict(yuy2, uv_stride=2 * w + 4), "uv_stride"), (dict(yuy2, y_stride=2 * w - 2, uv_stride=2 * w - 2), "y_stride"),
                    (dict(yuy2, u_offset=1, v_offset=2), "(1, 2)"), (dict(yuy2, u_offset=0, v_offset=1), "YUY2"), (dict(yuy2, u_offset=5, v_offset=7), "(5, 7)")):
        code, msg = _v(hostcheck, R.S422P, w, h, **f)
        assert code == 1 and word in msg and msg.startswith("yuv422 packed"), (f, msg)
    code, msg = _v(hostcheck, R.S422P, w + 1, h, **dict(yuy2, y_stride=2 * w + 4, uv_stride=2 * w + 4))
    assert code == 5 and "even" in msg
    assert _v(hostcheck, R.S422P, w, h, bps=2, **dict(yuy2, y_stride=4 * w, uv_stride=4 * w))[0] == 5
    # a packed layout under 422, a planar one under packed
    code, msg = _v(hostcheck, R.S422, w, h, **yuy2)
    assert code == 1 and "uv_step 4" in msg and msg.startswith("yuv422 layout")
    assert _v(hostcheck, R.S422P, w, h, **_asdict(R.make_layout(capi, "nv16", w, h)[0]))[0] == 1


# the 4:2:0 rules' messages as they stood before the sampling existed (csrc/frame_settings.h yuv420_validate), at 64 x 36
MESSAGES_420 = [
    (1, dict(y_stride=62), "yuv420 layout: y_stride 62 < width 64"),
    (1, dict(uv_stride=62), "yuv420 layout: uv_stride 62 < 64 (width/2 chroma samples of 2 bytes' step)"),
    (1, dict(uv_step=3), "yuv420 layout: uv_step 3 is neither 1 (planar) nor 2 (interleaved)"),
    (1, dict(uv_step=4), "yuv420 layout: uv_step 4 is neither 1 (planar) nor 2 (interleaved)"),
    (1, dict(u_offset=-1), "yuv420 layout: negative plane offset"),
    (1, dict(v_offset=2306), "yuv420 layout: interleaved chroma needs |v_offset - u_offset| == 1 (got 2304, 2306)"),
    (1, dict(u_offset=640, v_offset=641), "yuv420 layout: the UV plane [640, 1792) overlaps the Y plane [0, 2304)"),
    (1, dict(frame_stride=3454), "yuv420: frame_stride 3454 does not cover the frame's furthest byte (3456)"),
]
MESSAGES_420_16 = [
    (2, dict(y_stride=64, uv_stride=64, u_offset=2304, v_offset=2305), "yuv420 layout: y_stride 64 < 2 * width 64 (16-bit containers: strides are bytes)"),
    (2, dict(uv_stride=126), "yuv420 layout: uv_stride 126 < 128 (width/2 chroma samples of 2 * 2 bytes' step, 16-bit containers)"),
    (2, dict(y_stride=129), "yuv420 layout: 16-bit containers need even strides (y_stride 129, uv_stride 128)"),
    (2, dict(u_offset=4609, v_offset=4611), "yuv420 layout: 16-bit containers need even offsets (u_offset 4609, v_offset 4611)"),
    (2, dict(frame_stride=6913), "yuv420: 16-bit containers need an even frame_stride (6913)"),
    (2, dict(v_offset=4612), "yuv420 layout: interleaved chroma of 16-bit containers needs |v_offset - u_offset| == 2 (got 4608, 4612)"),
]


def test_all_420_messages_unchanged(hostcheck):
    w, h = 64, 36
    for bps, f, want in MESSAGES_420 + MESSAGES_420_16:
        a = dict(y_stride=w * bps, uv_stride=w * bps, u_offset=w * h * bps, v_offset=w * h * bps + bps, uv_step=2, frame_stride=-1)
        a.update(f)
        fs = a.pop("frame_stride")
        assert _v(hostcheck, 0, w, h, bps, fs=fs, **a) == (1, want), f
    good = dict(y_stride=w, uv_stride=w, u_offset=w * h, v_offset=w * h + 1, uv_step=2)
    assert _v(hostcheck, 0, w, h, **good) == (0, str(w * h * 3 // 2))
    assert _v(hostcheck, 0, w + 1, h, **good) == (5, "yuv420: width and height must be even (65x36), as cvtColor requires")
    assert _v(hostcheck, 0, 0, h, **good) == (1, "bad image geometry w=0 h=36")
    # the words the existing 4:2:0 and description tests match on
    for _, _, msg in MESSAGES_420 + MESSAGES_420_16:
        assert any(k in msg for k in ("y_stride", "uv_stride", "uv_step", "negative", "== 1", "== 2", "overlaps", "frame_stride", "even strides", "even offsets"))


def _cases(capi):
    """(sampling, w, h, fmt, depth, layout name, layout, frame bytes) over the GPU test's matrix."""
    for s in R.SAMPLINGS:
        for w, h in R.sizes(s):
            for depth in R.DEPTHS[s]:
                for fmt in R.FORMATS[s]:
                    for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                        yield s, w, h, fmt, depth, name, L, fb


def _run_case(exe, tmp, s, w, h, desc, L, fb, n, ofs, seed):
    frames = np.stack([R.random_frame(w, h, L, fb, desc[2], s, seed + i) for i in range(n)])
    cin, cout = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<12i3q", w, h, n, desc[0], desc[1], desc[2], s, L.y_stride, L.uv_stride, L.uv_step, ofs, 0, L.u_offset, L.v_offset, fb))
        f.write(frames.tobytes())
    flags = subprocess.check_output([exe, "convert", cin, cout]).decode()
    got = np.fromfile(cout, np.uint8).reshape(n, h, w, 3)
    for i in range(n):
        want = R.to_bgr(frames[i], w, h, L, desc, s)
        assert np.array_equal(got[i], want), (s, w, h, desc, ofs, i, flags, np.argwhere(got[i] != want)[:4])
    return flags


def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(capi, hostcheck, tmp_path):
    """Every case once under (BT601, LIMITED) and once under (BT709, FULL); two frames each; the source at an aligned base.  Every
    wide load and its fallback were taken."""
    seen = set()
    for k, (s, w, h, fmt, depth, name, L, fb) in enumerate(_cases(capi)):
        for m, r in ((D.BT601, D.LIMITED), (D.BT709, D.FULL)):
            flags = _run_case(hostcheck, tmp_path, s, w, h, (m, r, depth), L, fb, 2, 0, k)
        seen.update((s, depth, L.uv_step, word) for word in re.findall(r"\w+ \d+", flags))
    for s in R.SAMPLINGS:
        for depth in R.DEPTHS[s]:
            for step in ((4,) if s == R.S422P else (1, 2)):
                want = ["out4 0", "out4 1"]
                want += ["wide_y 0", "wide_y 4", "wide_y 8"] if s == R.S422P else ["wide_y 0", "wide_y 1"]
                if s != R.S422P:
                    want += ["wide_c 0", "wide_c 4", "wide_c 8"] if (s == R.S444 and step == 2) else ["wide_c 0", "wide_c 1"]
                for word in want:
                    assert (s, depth, step, word) in seen, (s, depth, step, word)


def test_sanitized_host_build_over_the_whole_matrix(capi, hostcheck_san, tmp_path):
    """One pair per case, rotating, and the source's base at 0, 2, 4 (8-bit: and 1) or 8 bytes past the alignment: address and
    undefined-behaviour checks on exact-size buffers — a wide load at an address that is not a multiple of its size, a load past
    the last sample or a store past the image would be reported."""
    for k, (s, w, h, fmt, depth, name, L, fb) in enumerate(_cases(capi)):
        m, r = D.PAIRS[k % 4]
        ofs = (0, 2, 4, 1)[(k // 4) % 4] if depth == D.D8 else (0, 2, 4, 8)[(k // 4) % 4]
        _run_case(hostcheck_san, tmp_path, s, w, h, (m, r, depth), L, fb, 1 + k % 2, ofs, k)
