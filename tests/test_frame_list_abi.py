"""Frame lists (include/slideo_amd.h "Frame lists") without a GPU: the header text, the 56-byte record and the exports at ABI 7 with
every existing record size unchanged, the NULL returns, the mirrors and the docs; and tools/frame_list_hostcheck.cpp, a stand-alone
program over csrc/frame_settings.h and csrc/frame_list.hip.h built plain and with -fsanitize=address,undefined and run as a program:
the gather's per-thread body lane by lane over the launch grid against a byte-for-byte restatement over the matrix, the load paths
taken, the staged layout of every case against the tight layout of its format class, and every rule with its code and message."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_match_frames_list", "slideo_match_frames_submit_list", "slideo_match_changed_frames_list",
       "slideo_match_changed_frames_submit_list", "slideo_changed_mask_list", "slideo_matcher_observe_frames_list",
       "slideo_matcher_gate_reset_from_frame_list", "slideo_group_match_frames_list", "slideo_group_match_changed_frames_list",
       "slideo_group_changed_mask_list", "slideo_frame_list_to_bgr8"]


def test_header_declares_the_record_and_the_calls():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    assert re.search(r"#define SLIDEO_FRAME_LIST_BGR\s+0\b", h) and re.search(r"#define SLIDEO_FRAME_LIST_YUV\s+1\b", h)
    assert "#define SLIDEO_ABI_VERSION 7" in h
    rec = re.search(r"typedef struct slideo_frame_list \{(.*?)\} slideo_frame_list;", h, re.S).group(1)
    assert re.search(r"int32_t door, on_device, n_frames, width, height, uv_step;", rec)
    assert re.search(r"int64_t stride\[3\];", rec) and re.search(r"const void\* const\* planes;", rec)
    sec = h.split("---- Frame lists", 1)[1].split("#define SLIDEO_FRAME_LIST_BGR", 1)[0]
    for word in ("bit for bit", "planes[3i + 1] + cy * stride[1]", "packed 4:2:2", "NULL", "alias or repeat", "copied at the call",
                 "read-in-place", "frame_gather_kernel", "page-locked", "a list of one", "primed from the list entry", "ABI stays 7",
                 "flipped"):
        assert word in sec, word


def test_library_exports_them_at_abi_7_and_no_record_changed(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.FrameListRec) == 56
    assert capi.FrameListRec.stride.offset == 24 and capi.FrameListRec.planes.offset == 48
    assert C.sizeof(capi.Yuv420Layout) == 32 and C.sizeof(capi.Config) == 168 and C.sizeof(capi.OcvVariants) == 36
    assert capi.VERDICT_DTYPE.itemsize == 16 and capi.KEYPOINT_DTYPE.itemsize == 24
    assert (capi.FRAME_LIST_BGR, capi.FRAME_LIST_YUV) == (0, 1)


def test_null_handles_and_null_records(capi):
    L = capi.lib()
    rec = capi.FrameListRec()
    buf = (C.c_uint8 * 64)()
    t = C.c_int64()
    r = C.byref(rec)
    assert L.slideo_match_frames_list(None, r, buf, None) == 1
    assert L.slideo_match_frames_submit_list(None, r, None, C.byref(t)) == 1
    assert L.slideo_match_changed_frames_list(None, r, buf, None, buf, None) == 1
    assert L.slideo_match_changed_frames_submit_list(None, r, None, C.byref(t)) == 1
    assert L.slideo_changed_mask_list(None, r, None, None, buf, None) == 1
    assert L.slideo_matcher_observe_frames_list(None, r, None) == 1
    assert L.slideo_matcher_gate_reset_from_frame_list(None, r, None) == 1
    assert L.slideo_group_match_frames_list(None, r, buf) == 1
    assert L.slideo_group_match_changed_frames_list(None, r, buf, None, buf) == 1
    assert L.slideo_group_changed_mask_list(None, r, None, None, buf, None) == 1
    assert L.slideo_frame_list_to_bgr8(None, r, buf, 64) == 1


def test_python_builder_fills_the_record(capi):
    import numpy as np
    w, h = 18, 10
    y = [np.zeros((h, w + 6), np.uint8)[:, :w] for _ in range(2)]
    c = [np.zeros((h // 2, w + 2), np.uint8)[:, :w] for _ in range(2)]
    fl = capi.frame_list([(y[i], c[i]) for i in range(2)], "yuv", w, h, chroma="vu")
    r = fl.rec
    assert (r.door, r.on_device, r.n_frames, r.width, r.height, r.uv_step) == (1, 0, 2, w, h, 2)
    assert list(r.stride) == [w + 6, w + 2, w + 2]
    assert [fl.table[k] for k in range(6)] == [y[0].ctypes.data, c[0].ctypes.data + 1, c[0].ctypes.data,
                                               y[1].ctypes.data, c[1].ctypes.data + 1, c[1].ctypes.data]
    imgs = [np.zeros((h, w, 4), np.uint8) for _ in range(3)]
    fl = capi.frame_list(imgs)
    assert (fl.rec.door, fl.rec.n_frames, fl.rec.width, fl.rec.height, fl.rec.stride[0]) == (0, 3, w, h, 4 * w)
    assert fl.table[1] is None and fl.table[2] is None and fl.table[3] == imgs[1].ctypes.data
    fl = capi.frame_list([np.zeros((3, h, w), np.uint8)], planar=True)
    assert (fl.rec.width, fl.rec.height, list(fl.rec.stride)) == (w, h, [w, w, w]) and fl.table[2] == fl.table[0] + 2 * w * h
    fl = capi.frame_list([np.zeros((h, 2 * w), np.uint8)], "yuv", w, h, chroma="uyvy")
    assert fl.rec.uv_step == 4 and (fl.table[1] - fl.table[0], fl.table[2] - fl.table[0]) == (0, 2)
    with pytest.raises(ValueError):
        capi.frame_list([np.zeros((h, w, 3), np.uint8), np.zeros((h, w + 1, 3), np.uint8)[:, :w]])      # one stride per plane
    with pytest.raises(ValueError):
        capi.frame_list([np.zeros((h, w, 3), np.uint8)[:, ::2]])                                        # rows not contiguous


def test_mirrors_and_docs():
    from slideo_amd import _capi as capi
    for cls in (capi.Matcher, capi.Group):
        for name in ("match_frames_list", "match_changed_frames_list", "changed_mask_list"):
            assert hasattr(cls, name), (cls, name)
    for name in ("submit_list", "submit_changed_list", "observe_frames_list", "gate_reset_from_frame_list", "frame_list_to_bgr8"):
        assert hasattr(capi.Matcher, name), name
    task = open(os.path.join(ROOT, "slideo_amd", "matching.py")).read()
    assert "Frame lists" in task and "_capi._FrameCalls" in task
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "slideo_frame_list" in hpp and "match_frames_list" in hpp
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "pub struct slideo_frame_list" in ffi
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    for f, needle in (("docs/EXTENSIONS.md", "## Frame lists"), ("README.md", "frame list"), ("INTEGRATION.md", "slideo_match_frames_list"),
                      ("README.md", "frame_list.hip.h")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)
    build = open(os.path.join(ROOT, "slideo_amd", "build.py")).read()
    assert build.count('"frame_list.hip.h"') == 1                  # compiled by exactly one stage unit
    units = [u for u in os.listdir(os.path.join(ROOT, "slideo_amd", "csrc")) if u.endswith(".hip")]
    assert [u for u in units if '#include "frame_list.hip.h"' in open(os.path.join(ROOT, "slideo_amd", "csrc", u)).read()] == ["stage_orb.hip"]


# ---- tools/frame_list_hostcheck.cpp ---------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "frame_list_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_list"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("frame_list_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


YUV_FORMS = {("420", 0): "i420", ("420", 1): "nv12", ("420", 2): "nv21", ("422", 0): "i422", ("422", 1): "nv16", ("422", 2): "nv61",
             ("444", 0): "i444", ("444", 1): "nv24", ("444", 2): "nv42",
             ("422_packed", 3): "yuy2", ("422_packed", 4): "yvyu", ("422_packed", 5): "uyvy", ("422_packed", 6): "vyuy"}


def _matrix(exe):
    p = subprocess.run([exe, "matrix"], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    lines = p.stdout.strip().split("\n")
    cases = [l.split(" ", 11) for l in lines if l.startswith("case ")]
    paths = [int(x) for x in lines[-1].split()[1:]]
    assert lines[-1].startswith("paths ") and len(cases) == len(lines) - 1
    return cases, paths


def _check_matrix(capi, cases, paths):
    seen = set()
    for _, door, sampling, depth, form, w, h, ofs, pad, n, verdict, rest in cases:
        form, w, h, ofs, pad, n = int(form), int(w), int(h), int(ofs), int(pad), int(n)
        bps = 1 if door == "bgr" or depth == "8" else 2
        seen.add((door, sampling, depth, form, w, h, ofs, pad, n))
        if bps == 2 and ofs % 2:                                  # an odd address in a 16-bit container
            assert verdict == "refused" and rest.startswith("1 ") and "even addresses" in rest, rest
            continue
        assert verdict == "ok", (door, sampling, depth, form, w, h, ofs, pad, n, rest)
        y_stride, uv_stride, u_off, v_off, uv_step, frame_bytes, stride = (int(x) for x in rest.split())
        if door == "bgr":
            bpp, planes = capi.pixel_format_info(form)
            assert (stride, frame_bytes) == (bpp * w, planes * h * bpp * w)
            continue
        T, fb = capi.yuv_layout(YUV_FORMS[(sampling, form)], w, h, bytes_per_sample=bps)
        assert (y_stride, uv_stride, u_off, v_off, uv_step, frame_bytes) == (T.y_stride, T.uv_stride, T.u_offset, T.v_offset, T.uv_step, fb)
        if sampling in ("420", "422_packed"):                     # ... and the library's own packed layout of the class
            P = capi.yuv420_layout_packed(YUV_FORMS[(sampling, form)], w, h, bps) if sampling == "420" else \
                capi.yuv_layout_packed(YUV_FORMS[(sampling, form)], w, h, bps)
            assert (P.y_stride, P.uv_stride, P.u_offset, P.v_offset, P.uv_step) == (y_stride, uv_stride, u_off, v_off, uv_step)
    # the whole matrix was walked
    want = set()
    for sampling in ("420", "422", "444"):
        for depth in ("8", "10_msb", "10_lsb"):
            for form in (0, 1, 2):
                want |= {("yuv", sampling, depth, form)}
    want |= {("yuv", "422_packed", "8", f) for f in (3, 4, 5, 6)} | {("bgr", "420", "8", f) for f in (0, 2, 6)}
    assert {c[:4] for c in seen} == want
    for door, sampling, depth, form in want:
        sizes = [(18, 10), (66, 34)] + ([(17, 9)] if door == "bgr" or sampling == "444" else [])
        for w, h in sizes:
            for ofs in (0, 1, 2, 4, 8, 16):
                for pad in (0, 2):
                    for n in (1, 2):
                        assert (door, sampling, depth, form, w, h, ofs, pad, n) in seen
    rows16, rows4, rows1, heads, tails = paths
    assert rows16 > 0 and rows4 > 0 and rows1 > 0 and heads > 0 and tails > 0, paths


def test_gather_body_over_the_matrix_against_the_restatement(capi, hostcheck):
    _check_matrix(capi, *_matrix(hostcheck))


def test_sanitized_host_build_over_the_whole_matrix(capi, hostcheck, hostcheck_san):
    cases, paths = _matrix(hostcheck_san)
    _check_matrix(capi, cases, paths)
    plain_cases, _ = _matrix(hostcheck)
    assert [c[:11] for c in cases] == [c[:11] for c in plain_cases]


RULES = {
    "null_record": (1, "null record"), "null_array": (1, "null planes array"), "needed_plane_null": (1, "needed and NULL"),
    "needed_plane_null_bgr": (1, "needed and NULL"), "unneeded_plane_set": (1, "not NULL"), "door": (1, "door 2"),
    "on_device": (1, "on_device 2"), "n_frames_negative": (1, "negative"), "stride_small_y": (1, "row bytes 18"),
    "stride_small_c": (1, "row bytes 9"), "stride_small_bgr": (1, "row bytes 54"), "stride_negative": (1, "negative"),
    "odd_address_16bit": (1, "even addresses"), "odd_stride_16bit": (1, "even strides"), "interleaved_distance": (1, "== +-1"),
    "interleaved_distance_16bit": (1, "== +-2"), "interleaved_order_differs": (1, "another U / V order"),
    "interleaved_strides": (1, "stride[1] == stride[2]"), "packed_pair": (1, "(u_offset, v_offset) = (1, 2)"),
    "packed_pair_differs": (1, "valid pair is (1, 3)"), "packed_strides": (1, "one plane"), "uv_step": (1, "uv_step 4"),
    "uv_step_packed": (1, "uv_step 2"), "size_odd_420": (5, "must be even"), "size_odd_width_packed": (5, "width must be even"),
    "size_limit": (5, "outside 1.."), "size_zero_bgr": (1, "bad image geometry"), "planar_rgb_plane_null": (1, "needed and NULL"),
}


@pytest.mark.parametrize("which", ["hostcheck", "hostcheck_san"])
def test_every_rule_is_refused_by_name_and_the_accepted_state_stays(request, which):
    exe = request.getfixturevalue(which)
    p = subprocess.run([exe, "rules"], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    lines = p.stdout.strip().split("\n")
    got = {}
    for i, l in enumerate(lines):
        if l.startswith("state "):
            assert l == "state same", lines[i - 1]
            continue
        name, code, msg = l.split(" ", 2)
        got[name] = (int(code), msg)
    assert set(got) == set(RULES)
    assert sum(l == "state same" for l in lines) == len(RULES) - 1     # (the null record has no accepted twin)
    for name, (code, word) in RULES.items():
        assert got[name][0] == code and word in got[name][1], (name, got[name])
