"""YUV chroma filter (include/slideo_amd.h "YUV chroma filter") without a GPU: the exports and the weight tables of all sixteen
(filter, sampling) pairs, the setter's rules (through tools/yuv_chroma_hostcheck.cpp, a stand-alone program over
csrc/frame_settings.h), the Python ValueErrors, a closed-form case, NEAREST through the restatement against the two earlier
restatements, and the kernel's per-thread body compiled for the host — with and without -fsanitize=address,undefined — against
tests/yuv_chroma_ref.py over the matrix of the GPU test."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import yuv_chroma_ref as R
import yuv_desc_ref as D
import yuv_sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_yuv_chroma", "slideo_matcher_yuv_chroma", "slideo_group_set_yuv_chroma", "slideo_yuv_chroma_weights"]
VALUES = (("NEAREST", 0), ("BILINEAR_LEFT", 1), ("BILINEAR_CENTER", 2), ("BILINEAR_TOPLEFT", 3))
# the header's table, written out: [parity][k-1, k, k+1]
COSITED, CENTRED, NONE = ((0, 4, 0), (0, 2, 2)), ((1, 3, 0), (0, 3, 1)), ((0, 4, 0), (0, 4, 0))


def test_header_declares_the_calls_and_constants():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    for name, v in VALUES:
        assert re.search(r"#define SLIDEO_YUV_CHROMA_%s\s+%d\b" % (name, v), h), name
    assert "#define SLIDEO_ABI_VERSION 7" in h
    sec = h.split("---- YUV chroma filter", 1)[1].split("/* ----", 1)[0]
    for word in ("DEPARTURE", "Contract", "co-sited", "centred", "+ 8) >> 4", "+ 2) >> 2", "clamped", "coincide", "changes nothing", "BGR calls never"):
        assert word in sec, word
    # struck from the sampling section's out-of-scope list
    samp = h.split("---- YUV sampling", 1)[1].split("/* ----", 1)[0]
    assert "chroma siting other than nearest;" not in samp


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
    out = (C.c_int32 * 12)()
    assert L.slideo_matcher_set_yuv_chroma(None, 0) == 1
    assert L.slideo_group_set_yuv_chroma(None, 0) == 1
    assert L.slideo_matcher_yuv_chroma(None, C.byref(v)) == 1
    assert L.slideo_yuv_chroma_weights(1, 0, None) == 1
    for f, s in ((-1, 0), (4, 0), (0, -1), (0, 4), (16, 1)):
        assert L.slideo_yuv_chroma_weights(f, s, out) == 1, (f, s)


def _expected(filt, sampling):
    if filt == R.NEAREST or sampling == R.S444:
        return NONE, NONE
    wh = CENTRED if filt == R.CENTER else COSITED
    if sampling != R.S420:
        return wh, NONE
    return wh, (COSITED if filt == R.TOPLEFT else CENTRED)


def test_weight_tables_of_all_sixteen_pairs(capi):
    for filt in (R.NEAREST, R.LEFT, R.CENTER, R.TOPLEFT):
        for sampling in (R.S420, R.S422, R.S444, R.S422P):
            got = capi.yuv_chroma_weights(filt, sampling)
            assert got == _expected(filt, sampling), (filt, sampling, got)
            assert got == R.weights(filt, sampling)
            for table in got:
                assert all(sum(row) == 4 for row in table)
    # by name; 4:2:2: LEFT and TOPLEFT coincide
    assert capi.yuv_chroma_weights("left", "420") == (COSITED, CENTRED)
    assert capi.yuv_chroma_weights("center", "420") == (CENTRED, CENTRED)
    assert capi.yuv_chroma_weights("topleft", "420") == (COSITED, COSITED)
    assert capi.yuv_chroma_weights("left", "422") == capi.yuv_chroma_weights("topleft", "422") == (COSITED, NONE)
    assert capi.yuv_chroma_weights("center", "422_packed") == (CENTRED, NONE)


def test_names_and_python_value_errors(capi):
    assert capi.YUV_CHROMA_FILTERS == {"nearest": 0, "left": 1, "center": 2, "topleft": 3}
    assert [capi.yuv_chroma_value(n) for n in ("nearest", "LEFT", "Center", "topleft", 3, np.int32(2))] == [0, 1, 2, 3, 3, 2]
    for bad in ("centre", "bilinear", "", None, 1.5, True, (1,)):
        with pytest.raises(ValueError):
            capi.yuv_chroma_value(bad)
    with pytest.raises(ValueError):
        capi.yuv_chroma_weights("middle", "420")
    with pytest.raises(ValueError):
        capi.yuv_chroma_weights("left", "411")
    with pytest.raises(capi.SlideoError):
        capi.yuv_chroma_weights(7, 0)


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(yuv_chroma="left")._yuv_chroma == "left"
    assert mt.HipImageVideoMatcher()._yuv_chroma is None
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_yuv_chroma") and hasattr(cls, "yuv_chroma")
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_yuv_chroma" in hpp and "slideo_group_set_yuv_chroma" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "yuv_chroma" in rs and "slideo_group_set_yuv_chroma" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    for name, v in VALUES:
        assert re.search(r"pub const SLIDEO_YUV_CHROMA_%s: i32 = %d;" % (name, v), ffi), name


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## YUV chroma filter"), ("README.md", "set_yuv_chroma"), ("INTEGRATION.md", "slideo_group_set_yuv_chroma"),
                      ("README.md", "yuv_chroma.hip.h")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------

# A 4x4 4:2:0 frame (chroma 2x2) with chroma sample (row 0, column 1) at 255 and the rest 0: U8 of every pixel by hand.
#   horizontal, row of samples (0, 255), H in quarters of 255 at x = 0..3:   co-sited (0, 2, 4, 4)   centred (0, 1, 3, 4)
#   vertical, rows (r0, 0), weights in quarters at y = 0..3:                 co-sited (4, 2, 0, 0)   centred (4, 3, 1, 0)
#   U8 = (wv * H * 255 + 8) >> 4
def _hand(hq, vq):
    return [[(v * q * 255 + 8) >> 4 for q in hq] for v in vq]


CLOSED_FORM = {
    R.LEFT: _hand((0, 2, 4, 4), (4, 3, 1, 0)),
    R.CENTER: _hand((0, 1, 3, 4), (4, 3, 1, 0)),
    R.TOPLEFT: _hand((0, 2, 4, 4), (4, 2, 0, 0)),
    R.NEAREST: _hand((0, 0, 4, 4), (4, 4, 0, 0)),
}


def test_closed_form_4x4():
    Cp = np.array([[0, 255], [0, 0]], np.int64)
    # the tables written out, so that a slip in _hand itself shows
    assert CLOSED_FORM[R.LEFT] == [[0, 128, 255, 255], [0, 96, 191, 191], [0, 32, 64, 64], [0, 0, 0, 0]]
    assert CLOSED_FORM[R.CENTER] == [[0, 64, 191, 255], [0, 48, 143, 191], [0, 16, 48, 64], [0, 0, 0, 0]]
    assert CLOSED_FORM[R.TOPLEFT] == [[0, 128, 255, 255], [0, 64, 128, 128], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert CLOSED_FORM[R.NEAREST] == [[0, 0, 255, 255], [0, 0, 255, 255], [0, 0, 0, 0], [0, 0, 0, 0]]
    for filt, want in CLOSED_FORM.items():
        got = R.chroma_at_pixels(Cp, filt, R.S420)
        assert got.tolist() == want, (filt, got.tolist())
    # 4:2:2: one row, no vertical step: (H + 2) >> 2
    row = np.array([[0, 255]], np.int64)
    assert R.chroma_at_pixels(row, R.LEFT, R.S422).tolist() == [[0, 128, 255, 255]]
    assert R.chroma_at_pixels(row, R.TOPLEFT, R.S422).tolist() == [[0, 128, 255, 255]]
    assert R.chroma_at_pixels(row, R.CENTER, R.S422P).tolist() == [[0, 64, 191, 255]]
    # 4:4:4: untouched
    assert R.chroma_at_pixels(Cp, R.LEFT, R.S444) is Cp


def test_a_flat_plane_stays_flat_and_the_range_needs_no_clamp():
    rng = np.random.default_rng(5)
    for sampling in R.SAMPLINGS:
        for filt in R.FILTERS:
            for v in (0, 1, 127, 255):
                assert np.all(R.chroma_at_pixels(np.full((3, 5), v, np.int64), filt, sampling) == v)
            out = R.chroma_at_pixels(rng.integers(0, 256, (7, 9), dtype=np.int64), filt, sampling)
            assert out.min() >= 0 and out.max() <= 255 and out.shape == ((14 if sampling == R.S420 else 7), 18)


def test_nearest_through_the_restatement_is_the_earlier_restatements(capi):
    """On yuv_desc_ref's and yuv_sampling_ref's own matrices."""
    k = 0
    for (w, h) in D.SIZES:
        for depth in D.DEPTHS:
            for fmt in D.FORMATS:
                for name, L, fb in D.layouts(capi, fmt, w, h, depth):
                    m, r = D.PAIRS[k % 4]
                    k += 1
                    buf = D.random_frame(w, h, L, fb, depth, k)
                    assert np.array_equal(R.to_bgr(buf, w, h, L, (m, r, depth), R.S420, R.NEAREST), D.to_bgr(buf, w, h, L, (m, r, depth)))
    for s in S.SAMPLINGS:
        for (w, h) in S.sizes(s):
            for depth in S.DEPTHS[s]:
                for fmt in S.FORMATS[s]:
                    for name, L, fb in S.layouts(capi, fmt, w, h, depth):
                        m, r = D.PAIRS[k % 4]
                        k += 1
                        buf = S.random_frame(w, h, L, fb, depth, s, k)
                        assert np.array_equal(R.to_bgr(buf, w, h, L, (m, r, depth), s, R.NEAREST), S.to_bgr(buf, w, h, L, (m, r, depth), s))
                        if s == S.S444:     # and 4:4:4 under a filter is 4:4:4
                            assert np.array_equal(R.to_bgr(buf, w, h, L, (m, r, depth), s, R.LEFT), S.to_bgr(buf, w, h, L, (m, r, depth), s))


# ---- tools/yuv_chroma_hostcheck.cpp -----------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "yuv_chroma_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_chroma"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_chroma_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _lines(exe, *args):
    out = subprocess.check_output([exe] + [str(a) for a in args]).decode().strip().split("\n")
    return [(int(l.partition(" ")[0]), l.partition(" ")[2]) if not l.startswith("state") else tuple(int(x) for x in l.split()[1:]) for l in out]


def test_host_weight_rule_is_the_library_s(capi, hostcheck):
    for filt in range(4):
        for sampling in range(4):
            out = subprocess.check_output([hostcheck, "weights", str(filt), str(sampling)]).decode().split()
            assert [int(x) for x in out] == [0] + R.weights12(filt, sampling)
    assert subprocess.check_output([hostcheck, "weights", "4", "0"]).decode().split()[0] == "1"


def test_setter_refusals_and_the_state_each_leaves(hostcheck):
    for v in (0, 1, 2, 3):
        assert _lines(hostcheck, "set", "c", v) == [(0, "ok"), (0, 0, 0, 0, v)]
    for bad in (4, -1, 16):
        (code, msg), state = _lines(hostcheck, "set", "c", 2, "c", bad)[1:]
        assert code == 1 and "yuv chroma filter" in msg and str(bad) in msg and state == (0, 0, 0, 0, 2)
    # the description's and the sampling's setters leave the filter alone, and the other way round
    assert _lines(hostcheck, "set", "c", 1, "d", 1, 1, 2, "s", 1)[-1] == (1, 1, 2, 1, 1)
    assert _lines(hostcheck, "set", "d", 1, 0, 1, "s", 2, "c", 3)[-1] == (1, 0, 1, 2, 3)
    # a refused description or sampling leaves everything, the filter included
    assert _lines(hostcheck, "set", "c", 3, "d", 2, 0, 0, "s", 9)[-1] == (0, 0, 0, 0, 3)
    # the filter is accepted under every sampling, 4:4:4 and packed included, and does not touch the packed / 10-bit rule
    for s in (0, 1, 2, 3):
        assert _lines(hostcheck, "set", "s", s, "c", 1)[-1] == (0, 0, 0, s, 1)
    a = _lines(hostcheck, "set", "s", 3, "c", 2, "d", 0, 0, 1)
    assert a[2][0] == 5 and a[3] == (0, 0, 0, 3, 2)
    # back to nearest
    assert _lines(hostcheck, "set", "c", 1, "c", 0)[-1] == (0, 0, 0, 0, 0)


def _write_cases(capi, path, pick_desc, n_of):
    """The GPU test's whole matrix as one case file; returns [(frames, w, h, L, desc, sampling, filter)]."""
    want = []
    with open(path, "wb") as f:
        for k, (s, depth, fmt, name, L, fb, w, h) in enumerate(R.tap_cases(capi)):
            m, r = pick_desc(k)
            filt = R.FILTERS[k % 3]
            n = n_of(k)
            frames = np.stack([R.random_frame(w, h, L, fb, depth, s, 3 * k + i) for i in range(n)])
            f.write(struct.pack("<12i3q", w, h, n, m, r, depth, s, L.y_stride, L.uv_stride, L.uv_step, filt, frames.size, L.u_offset, L.v_offset, fb))
            f.write(frames.tobytes())
            want.append((frames, w, h, L, (m, r, depth), s, filt, (fmt, name)))
    return want


def _check(exe, capi, tmp, pick_desc, n_of):
    cin, cout = str(tmp / "cases.bin"), str(tmp / "out.bin")
    want = _write_cases(capi, cin, pick_desc, n_of)
    text = subprocess.check_output([exe, "convert", cin, cout]).decode()
    hits = {k: int(v) for k, v in (l.split() for l in text.strip().split("\n"))}
    assert hits["records"] == len(want)
    got = np.fromfile(cout, np.uint8)
    at = 0
    for frames, w, h, L, desc, s, filt, tag in want:
        for fr in frames:
            img = got[at:at + w * h * 3].reshape(h, w, 3)
            at += w * h * 3
            ref = R.to_bgr(fr, w, h, L, desc, s, filt)
            assert np.array_equal(img, ref), (tag, w, h, desc, s, filt, np.argwhere(img != ref)[:4])
    assert at == got.size
    return hits


PATHS = ("wide_y", "bytes_y", "packed8", "packed4", "wide_c8", "wide_c4", "wide_c2", "bytes_c", "neighbour", "halo", "clamp", "out4", "out_bytes")


def test_host_build_of_the_kernel_body_equals_the_restatement(capi, hostcheck, tmp_path):
    """The whole matrix, two frames each, the filter and the colour pair rotating; every record at five source offsets.  Every wide
    load, its fallback, the neighbour path, the halo path and the clamp were taken."""
    hits = _check(hostcheck, capi, tmp_path, lambda k: D.PAIRS[(k // 3) % 4], lambda k: 2)
    for p in PATHS:
        assert hits[p] > 0, (p, hits)


def test_sanitized_host_build_over_the_whole_matrix(capi, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks on exact-size buffers at source offsets 0, 1, 2, 4 and 8: a wide load at an address
    that is not a multiple of its size, a load past the last sample (a halo or a clamped row read too far) or a store past the image
    would be reported.  A stand-alone program: nothing is loaded into Python."""
    hits = _check(hostcheck_san, capi, tmp_path, lambda k: D.PAIRS[(k // 3 + 1) % 4], lambda k: 1 + k % 2)
    for p in PATHS:
        assert hits[p] > 0, (p, hits)
