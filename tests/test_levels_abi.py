"""Frame levels (include/slideo_amd.h "Frame levels") without a GPU: the header, the exports at ABI 7, the mirrors, the pure call
slideo_frame_levels_lut against the restatement (tests/levels_ref.py) for all 32 640 (lo, hi) pairs and its refusals, the points
rule on hand-made histograms, the Python ValueErrors, and both kernels' per-thread bodies compiled for the host
(tools/levels_hostcheck.cpp) — with and without -fsanitize=address,undefined — against the restatement over the GPU test's sizes."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import levels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_frame_levels", "slideo_matcher_frame_levels", "slideo_group_set_frame_levels", "slideo_frame_levels_lut",
       "slideo_levels_bgr8", "slideo_matcher_levels_begin", "slideo_matcher_levels_end", "slideo_matcher_levels_info",
       "slideo_matcher_levels_histogram", "slideo_matcher_levels_points"]


def test_header_declares_the_calls():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    assert "#define SLIDEO_ABI_VERSION 7" in h
    sec = h.split("---- Frame levels", 1)[1].split("/* ---- Working size", 1)[0]
    for word in ("lut[c][in[y][x][c]]", "LAST step", "not levelled twice", "stored as off", "510 * (x - lo[c])", "floor(total * low_ppm / 1e6)",
                 "total - 1 - floor(total * high_ppm / 1e6)", "learnt on levelled frames", "DEPARTURE", "Out of scope", "gamma", "never written",
                 "levels_hist_kernel", "nothing is installed"):
        assert word in sec, word


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.Config) == 168


def test_null_handles_and_outputs(capi):
    L = capi.lib()
    v, q = C.c_int32(), C.c_int64()
    buf = (C.c_uint8 * 768)()
    assert L.slideo_matcher_set_frame_levels(None, buf) == 1
    assert L.slideo_group_set_frame_levels(None, buf) == 1
    assert L.slideo_matcher_frame_levels(None, buf, C.byref(v)) == 1
    assert L.slideo_levels_bgr8(None, buf, 2, 2, 6, buf, 64) == 1
    for name in ("begin", "end"):
        assert getattr(L, "slideo_matcher_levels_" + name)(None) == 1
    assert L.slideo_matcher_levels_info(None, C.byref(q), C.byref(q)) == 1
    assert L.slideo_matcher_levels_histogram(None, buf) == 1
    assert L.slideo_matcher_levels_points(None, 0, 0, buf, buf) == 1
    three = (C.c_int32 * 3)(0, 0, 0)
    assert L.slideo_frame_levels_lut(None, three, buf) == 1 and L.slideo_frame_levels_lut(three, None, buf) == 1
    assert L.slideo_frame_levels_lut(three, three, None) == 1


def test_frame_levels_lut_agrees_with_the_restatement_for_every_pair(capi):
    """All 32 640 pairs 0 <= lo < hi <= 255 through the library's pure call, three per call (one per channel)."""
    L = capi.lib()
    pairs = [(lo, hi) for lo in range(255) for hi in range(lo + 1, 256)]
    assert len(pairs) == 32640
    out = np.empty((3, 256), np.uint8)
    for i in range(0, len(pairs), 3):
        trio = pairs[i:i + 3]
        assert len(trio) == 3
        lo = (C.c_int32 * 3)(*[p[0] for p in trio])
        hi = (C.c_int32 * 3)(*[p[1] for p in trio])
        assert L.slideo_frame_levels_lut(lo, hi, out.ctypes.data_as(C.c_void_p)) == 0
        for c, (l, h) in enumerate(trio):
            assert np.array_equal(out[c], R.stretch_row(l, h)), (l, h)
    # the vectorised row is the restatement's scalar rule; the ends and the identity
    for l, h in ((0, 255), (34, 106), (0, 1), (254, 255), (17, 200)):
        assert np.array_equal(R.stretch_lut([l] * 3, [h] * 3)[0], R.stretch_row(l, h))
    assert np.array_equal(capi.frame_levels_lut(0, 255), R.identity())
    t = capi.frame_levels_lut([34, 0, 100], [106, 255, 101])
    assert np.array_equal(t, R.stretch_lut([34, 0, 100], [106, 255, 101]))
    assert t[0, 34] == 0 and t[0, 106] == 255 and t[0, 70] == 128 and t[2, 100] == 0 and t[2, 101] == 255


def test_frame_levels_lut_refusals_name_the_channel(capi):
    L = capi.lib()
    out = np.full((3, 256), 7, np.uint8)
    for c in range(3):
        for l, h in ((-1, 100), (0, 256), (100, 100), (101, 100), (255, 255)):
            lo, hi = [0, 0, 0], [255, 255, 255]
            lo[c], hi[c] = l, h
            assert L.slideo_frame_levels_lut((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi), out.ctypes.data_as(C.c_void_p)) == 1
            msg = L.slideo_last_error(None).decode()
            assert "channel %d" % c in msg and "BGR"[c] in msg and str(l) in msg, msg
            assert (out == 7).all()                              # nothing written
            with pytest.raises(ValueError) as e:
                capi.frame_levels_lut(lo, hi)
            assert "channel %d" % c in str(e.value)
    with pytest.raises(ValueError):
        capi.frame_levels_lut([0, 0], [255, 255])


def test_python_value_errors(capi):
    with pytest.raises(ValueError):
        capi._levels_table(np.zeros((3, 255), np.uint8))
    with pytest.raises(ValueError):
        capi._levels_table(np.full((3, 256), 256, np.int32))
    with pytest.raises(ValueError):
        capi._levels_table(np.zeros((3, 256), np.float32))
    assert capi._levels_table(np.arange(768) % 256).dtype == np.uint8
    assert capi._levels_table(R.identity().reshape(768)).shape == (3, 256)


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    lut = R.random_lut(1)
    assert mt.HipImageVideoMatcher(frame_levels=lut)._frame_levels is lut
    assert mt.HipImageVideoMatcher()._frame_levels is None
    assert callable(mt.learn_frame_levels)
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_frame_levels") and hasattr(cls, "frame_levels")
    for name in ("levels_bgr", "levels_begin", "levels_end", "levels_info", "levels_histogram", "levels_points"):
        assert hasattr(capi.Matcher, name), name
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_frame_levels" in hpp and "slideo_group_set_frame_levels" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "pub frame_levels:" in rs and "slideo_group_set_frame_levels" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name


def test_the_setting_commits_under_the_pixel_formats_row():
    src = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    body = re.search(r"enum Setting \{(.*?)\};", src, re.S).group(1)
    assert [n.strip() for n in body.replace("\n", " ").split(",")][-1] == "N_SETTINGS" and body.count("SET_") == 8
    for unit in ("capi_runtime.hip", "capi_group.hip"):
        text = open(os.path.join(ROOT, "slideo_amd", "csrc", unit)).read()
        assert re.search(r"SET_YUV_DESCRIPTION, \[&\]\(const FrameSettings& s\) \{ return propose_frame_levels\(s, lut768, ", text), unit
    rt = open(os.path.join(ROOT, "slideo_amd", "csrc", "capi_runtime.hip")).read()
    assert "on_device && !src.converted() && !pre" not in rt and "src.on_device && !src.kernel_in_front()" in rt


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## Frame levels"), ("README.md", "set_frame_levels"), ("README.md", "levels.hip.h"),
                      ("INTEGRATION.md", "slideo_group_set_frame_levels")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- tools/levels_hostcheck.cpp ---------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "levels_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("levels"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("levels_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_host_lut_rule_for_every_pair_and_its_refusals(hostcheck, tmp_path):
    out = str(tmp_path / "sweep.bin")
    assert subprocess.check_output([hostcheck, "lutsweep", out]).split()[0] == b"32640"
    got = np.fromfile(out, np.uint8).reshape(32640, 256)
    k = 0
    for lo in range(255):
        for hi in range(lo + 1, 256):
            assert np.array_equal(got[k], R.stretch_row(lo, hi)), (lo, hi)
            k += 1
    one = str(tmp_path / "lut.bin")
    assert subprocess.check_output([hostcheck, "lut", "0", "0", "0", "255", "255", "255", one]).decode().strip() == "0 ok identity 1"
    assert np.array_equal(np.fromfile(one, np.uint8).reshape(3, 256), R.identity())
    line = subprocess.check_output([hostcheck, "lut", "0", "9", "0", "255", "9", "255", one]).decode()
    assert line.startswith("1 ") and "channel 1 (G)" in line


def _points(exe, tmp, hist, low, high):
    path = str(tmp / "hist.bin")
    np.asarray(hist, np.uint64).reshape(768).tofile(path)
    return subprocess.check_output([exe, "points", str(low), str(high), path]).decode().strip()


def test_points_rule_on_hand_made_histograms(hostcheck, tmp_path):
    def both(hist, low, high):
        lo, hi = R.points(hist, low, high)
        assert _points(hostcheck, tmp_path, hist, low, high) == " ".join(str(v) for v in lo + hi), (low, high)
        return lo, hi
    # all mass in one bin: lo == hi == that bin whatever the cut (the LUT rule is what refuses it)
    h = np.zeros((3, 256), np.uint64)
    h[0, 255] = h[1, 0] = h[2, 77] = 1000
    for low, high in ((0, 0), (10000, 10000), (999999, 999999), (1000000, 1000000)):
        assert both(h, low, high) == ([255, 0, 77], [255, 0, 77])
    # ppm 0: the smallest and the largest sample
    h = np.zeros((3, 256), np.uint64)
    h[:, 10] = 1; h[:, 20] = 98; h[:, 250] = 1
    assert both(h, 0, 0) == ([10] * 3, [250] * 3)
    # ties at the rank: 100 samples, a cut of 1 % is rank 1 — the first sample of bin 20 — and rank 98, the last of bin 20
    assert both(h, 10000, 10000) == ([20] * 3, [20] * 3)
    assert both(h, 9999, 9999) == ([10] * 3, [250] * 3)          # floor(100 * 9999 / 1e6) = 0
    # the rank falls on the last sample of a bin / the first of the next
    h = np.zeros((3, 256), np.uint64)
    h[:, 5] = 50; h[:, 6] = 50
    assert both(h, 490000, 0)[0] == [5] * 3 and both(h, 500000, 0)[0] == [6] * 3
    assert both(h, 0, 490000)[1] == [6] * 3 and both(h, 0, 500000)[1] == [5] * 3
    # channels differ, and totals beyond 32 bits
    h = np.zeros((3, 256), np.uint64)
    h[0, 1] = 1 << 40; h[0, 200] = 1 << 40; h[1, 3] = 7; h[2, 0] = 1; h[2, 255] = (1 << 33) + 1
    assert both(h, 500000, 0) == ([200, 3, 255], [200, 3, 255])
    assert both(h, 1, 1) == ([1, 3, 255], [200, 3, 255])
    # refusals: a ppm out of range; an empty channel
    assert _points(hostcheck, tmp_path, h, -1, 0).startswith("1 ") and _points(hostcheck, tmp_path, h, 0, 1000001).startswith("1 ")
    h[1] = 0
    assert _points(hostcheck, tmp_path, h, 0, 0).startswith("4 ")


def _apply_case(exe, tmp, w, h, stride, n, sofs, dofs, in_place, seed, lut):
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, (n, h, stride), dtype=np.uint8)
    imgs = np.ascontiguousarray(buf[:, :, :3 * w]).reshape(n, h, w, 3)
    cin, cout = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<8i", w, h, n, stride, stride, sofs, dofs, 1 if in_place else 0))
        f.write(np.ascontiguousarray(lut, np.uint8).tobytes())
        f.write(buf.tobytes())
    flags = subprocess.check_output([exe, "apply", cin, cout]).decode()
    got = np.fromfile(cout, np.uint8)
    # the whole destination buffer: the levelled pixels, and between the rows the source's own bytes (in place) or the fill that
    # was there (out of place: never written)
    want = buf.copy() if in_place else np.full_like(buf, 0xAA)
    want[:, :, :3 * w] = R.apply(imgs, lut).reshape(n, h, 3 * w)
    assert got.size == (n * h - 1) * stride + 3 * w
    assert np.array_equal(got, want.reshape(-1)[:got.size]), (w, h, stride, sofs, in_place, flags)
    if not in_place:
        assert "src_unchanged 1" in flags
    return flags


def test_host_build_of_levels_thread_equals_the_restatement(hostcheck, tmp_path):
    """Every size and stride, in place and out of place, two frames: both loads and both stores were taken on either side."""
    seen = set()
    luts = [R.random_lut(3), R.stretch_lut([34] * 3, [106] * 3)]
    for k, (w, h) in enumerate(R.SIZES):
        for j, stride in enumerate(R.strides(w)):
            for in_place in (True, False):
                for sofs, dofs in ((0, 0), (4, 1)):
                    flags = _apply_case(hostcheck, tmp_path, w, h, stride, 2, sofs, dofs, in_place, 10 * k + j, luts[(k + j) % 2])
                    seen.update((in_place, word) for word in re.findall(r"(?:in4|out4) \d", flags))
    for place in (True, False):
        for word in ("in4 0", "in4 1", "out4 0", "out4 1"):
            assert (place, word) in seen, (place, word)
    assert (False, "in4 1") in seen                                # (and the mixed case: aligned loads, byte stores)


def test_sanitized_host_build_of_levels_thread(hostcheck_san, tmp_path):
    """Base offsets 0, 1, 2, 4 and 8 on exact-size heap buffers, in place and out of place, one or two frames: a dword access at
    an address that is not a multiple of 4, a load past the last pixel or a store outside the image would be reported."""
    lut = R.random_lut(4)
    for k, (w, h) in enumerate(R.SIZES):
        big = w * h > 100000
        for j, stride in enumerate(R.strides(w)):
            for i, ofs in enumerate((0, 1, 2, 4, 8)):
                if big and (i + j) % 3:
                    continue                                      # (the large size: every offset and stride once, not every pair)
                for in_place in (True, False):
                    _apply_case(hostcheck_san, tmp_path, w, h, stride, 1 + (k + i) % 2, ofs, (0, ofs)[(i + j) % 2], in_place, 100 + k, lut)


def _contents(name, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if name == "white":
        return np.full((n, h, w, 3), 255, np.uint8)
    if name == "alternating":
        f = np.empty((n, h, w, 3), np.uint8)
        f[0::2] = (12, 200, 90); f[1::2] = (13, 200, 91)
        return f
    if name == "static":
        return np.repeat(rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8) // 64 * 64, n, axis=0)
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _hist_case(exe, tmp, frames, stride, ofs, split=()):
    n, h, w, _ = frames.shape
    buf = np.random.default_rng(1).integers(0, 256, (n, h, stride), dtype=np.uint8)
    buf[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
    cin, cout = str(tmp / "hcase.bin"), str(tmp / "hout.bin")
    sp = list(split) + [0] * (4 - len(split))
    with open(cin, "wb") as f:
        f.write(struct.pack("<9i", w, h, n, stride, ofs, *sp))
        f.write(buf.tobytes())
    flags = subprocess.check_output([exe, "hist", cin, cout]).decode()
    got = np.fromfile(cout, np.uint64).reshape(3, 256)
    assert np.array_equal(got, R.histogram(frames)), (w, h, n, stride, ofs, split, flags)
    return flags


@pytest.mark.parametrize("san", [False, True])
def test_host_build_of_levels_hist_thread_equals_bincount(hostcheck, hostcheck_san, tmp_path, san):
    exe = hostcheck_san if san else hostcheck
    seen = set()
    k = 0
    for w, h in R.SIZES[:-1] + [(130, 1100)]:                      # (1100 rows: more tiles than LVH_GY, a block walks several)
        for name in ("white", "alternating", "static", "noise"):
            for n in (1, 4, 5, 9):
                if h > 1000 and n != 5:
                    continue
                stride = R.strides(w)[k % 3]
                ofs = (0, 1, 2, 4, 8)[k % 5]
                frames = _contents(name, n, h, w, k)
                flags = _hist_case(exe, tmp_path, frames, stride, ofs, () if k % 2 else (n // 2,))
                seen.update(re.findall(r"in4 \d", flags))
                if h > 1000:
                    assert "tiles 3" in flags and "grid_y 128" in flags
                k += 1
    assert seen == {"in4 0", "in4 1"}
