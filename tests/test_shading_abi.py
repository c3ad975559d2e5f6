"""Frame shading and the match shading map (include/slideo_amd.h "Frame shading", "Match shading map") without a GPU: the header, the
exports at ABI 7, the mirrors, the docs; the null-handle refusals; the pure call slideo_shading_field against the restatement
(tests/shading_ref.py) on named and random arrays and its refusals; the apply rule's edge cases; both kernels' bodies compiled for
the host (tools/shading_hostcheck.cpp) — with and without -fsanitize=address,undefined, run as a program — against the restatement:
shading_kernel's thread body lane by lane, shading_map_kernel's per-frame body block by block on the tone table's constructed cases,
whole and in row tiles of 7 rows, and on wild keypoints and transforms; and the use through the CPU restatement of the pipeline."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import evidence_ref as E
import levels_ref as LR
import shading_ref as R
import test_tone_abi as TA            # (the constructed cases as units of the CPU restatement, and the unit file both host checks read)
import tone_ref as T
from conftest import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_frame_shading", "slideo_matcher_frame_shading", "slideo_group_set_frame_shading", "slideo_shading_bgr8",
       "slideo_shading_field", "slideo_matcher_shading_begin", "slideo_matcher_shading_end", "slideo_matcher_shading_info",
       "slideo_matcher_shading_sums", "slideo_group_shading_begin", "slideo_group_shading_end", "slideo_group_shading_info",
       "slideo_group_shading_sums"]


# ---- exports, header, mirrors, docs ------------------------------------------------------------------------------------------------

def test_header_declares_the_calls():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    assert "#define SLIDEO_ABI_VERSION 7" in h
    sec = h.split("---- Frame shading", 1)[1].split("/* ---- Working size", 1)[0]
    for word in ("G = (L * (cell - fx) + R * fx + cell * cell / 2) >> (2 * log2(cell))", "min(255, (in[c] * G + 128) >> 8)", "stored as off",
                 "BEFORE the levels", "not shaded twice", "never written", "FAST corner", "one gain for all three", "fused", "DEPARTURE",
                 "multiplicative", "(2 * 4096 * sum_p + sum_f) / (2 * sum_f)", "(2 * S + 9) / 18", "(node + 8) >> 4", "nothing is installed",
                 "extrapolation"):
        assert word in sec, word
    sec = h.split("---- Match shading map", 1)[1]
    for word in ("k = (Yi / cell) * gw + Xi / cell", "cnt[k] += 1", "sum_f[k] += B + G + R", "sum_p[k] += B + G + R", "learn the field\n * first and the table second",
                 "4096 cells", "2^20 frames", "Verdict bytes are identical", "shading_map_kernel", "ratio of sums", "occluder", "Clipped highlights"[1:],
                 "FIXED camera", "cell 16 needs more frames", "SLIDEO_ERR_CAPACITY"):
        assert word in sec, word
    assert "SLIDEO_SHADING_MAX_FRAMES" in h.split(" * Environment", 1)[1].split("*/", 1)[0]


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.Config) == 168


def test_null_handles_and_outputs_write_nothing(capi):
    L = capi.lib()
    v = [C.c_int32(7) for _ in range(4)]
    g = np.full(4, 300, np.uint16)
    buf = np.full(64, 9, np.uint8)
    assert L.slideo_matcher_set_frame_shading(None, 16, 16, 16, g.ctypes.data_as(C.c_void_p)) == 1
    assert L.slideo_group_set_frame_shading(None, 16, 16, 16, g.ctypes.data_as(C.c_void_p)) == 1
    assert L.slideo_matcher_frame_shading(None, g.ctypes.data_as(C.c_void_p), C.c_int64(4), *[C.byref(x) for x in v]) == 1
    assert [x.value for x in v] == [7] * 4 and (g == 300).all()
    assert L.slideo_shading_bgr8(None, buf.ctypes.data_as(C.c_void_p), 2, 2, 6, buf.ctypes.data_as(C.c_void_p), C.c_int64(64)) == 1
    assert (buf == 9).all()
    one = np.ones((1, 1), np.uint64)
    out, used = np.full((2, 2), 5, np.uint16), C.c_int32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, p(one), p(one), p(out)), (p(one), None, p(one), p(out)), (p(one), p(one), None, p(out)), (p(one), p(one), p(one), None)):
        assert L.slideo_shading_field(args[0], args[1], args[2], 1, 1, 32, C.c_int64(1), 64, 2048, 0, args[3], C.byref(used)) == 1
    assert (out == 5).all() and used.value == 7
    assert L.slideo_shading_field(p(one), p(one), p(one), 1, 1, 32, C.c_int64(1), 64, 2048, 0, p(out), None) == 0      # cells_used may be null
    assert (out == 256).all()
    # the session's calls: a null handle (and, with a handle, a null output: tests/test_gpu_shading_map.py) writes nothing
    q = [C.c_int64(7) for _ in range(2)]
    w = [C.c_int32(7) for _ in range(8)]
    sums = np.full(4, 9, np.uint64)
    for who in ("matcher", "group"):
        assert getattr(L, "slideo_%s_shading_begin" % who)(None, 32, 0, 1, 255) == 1
        assert getattr(L, "slideo_%s_shading_end" % who)(None) == 1
        assert getattr(L, "slideo_%s_shading_info" % who)(None, *[C.byref(x) for x in w], C.byref(q[0])) == 1
        assert getattr(L, "slideo_%s_shading_sums" % who)(None, p(sums), p(sums), p(sums), C.c_int64(4), C.byref(w[0]), C.byref(w[1]), C.byref(q[0]),
                                                          C.byref(q[1])) == 1
    assert [x.value for x in w] == [7] * 8 and [x.value for x in q] == [7, 7] and (sums == 9).all()


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    f = (40, 20, 16, R.random_field(40, 20, 16, 1))
    assert mt.HipImageVideoMatcher(frame_shading=f)._frame_shading[3] is f[3]
    assert mt.HipImageVideoMatcher()._frame_shading is None
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_frame_shading") and hasattr(cls, "frame_shading")
    assert hasattr(capi.Matcher, "shading_bgr") and callable(capi.shading_field)
    for cls in (capi.Matcher, capi.Group):
        for name in ("shading_begin", "shading_end", "shading_info", "shading_sums"):
            assert callable(getattr(cls, name)), name
    import inspect
    sig = inspect.signature(mt.learn_frame_shading_from_matches)
    assert list(sig.parameters)[:2] == ["matcher", "frame_batches"]
    for name in ("cell", "min_inliers", "min_hits", "flat", "min_count", "min_gain", "max_gain", "smooth"):      # no parameter has a default
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is inspect.Parameter.empty, name
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_frame_shading" in hpp and "slideo_group_set_frame_shading" in hpp
    for name in ("void shading_begin(", "void shading_end(", "ShadingSums shading_info(", "ShadingSums shading_sums(", "static bool shading_field(",
                 "slideo_group_shading_begin", "slideo_group_shading_end", "slideo_group_shading_info", "slideo_group_shading_sums"):
        assert name in hpp, name
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "pub frame_shading:" in rs and "slideo_group_set_frame_shading" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name


def test_python_value_errors(capi):
    g = R.random_field(40, 20, 16, 2)
    assert capi._shading_field(40, 20, 16, g)[3].dtype == np.uint16
    assert capi._shading_field(40, 20, 16, g.astype(np.int64).reshape(-1))[3].shape == (3, 4)
    for bad in (lambda: capi._shading_field(40, 20, 8, g), lambda: capi._shading_field(41 + 16, 20, 16, g), lambda: capi._shading_field(0, 20, 16, g),
                lambda: capi._shading_field(40, 20, 16, g.astype(np.float32)), lambda: capi._shading_field(40, 20, 16, np.zeros((3, 4), np.uint16)),
                lambda: capi._shading_field(40, 20, 16, np.full((3, 4), 65536, np.int64))):
        with pytest.raises(ValueError):
            bad()


def test_the_setting_commits_under_the_levels_row_and_stands_in_front_of_them():
    src = open(os.path.join(ROOT, "slideo_amd", "csrc", "frame_settings.h")).read()
    body = re.search(r"enum Setting \{(.*?)\};", src, re.S).group(1)
    assert body.count("SET_") == 8                                 # enum Setting does not grow
    for unit in ("capi_runtime.hip", "capi_group.hip"):
        text = open(os.path.join(ROOT, "slideo_amd", "csrc", unit)).read()
        assert re.search(r"SET_YUV_DESCRIPTION, \[&\]\(const FrameSettings& s\) \{ return propose_frame_shading\(s, aw, ah, cell, gains\)", text), unit
    rt = open(os.path.join(ROOT, "slideo_amd", "csrc", "runtime.hpp")).read()
    assert "plan.prep != PREP_NONE || shading || levels || list" in rt                # FrameSrc::kernel_in_front() knows of it
    stage = open(os.path.join(ROOT, "slideo_amd", "csrc", "capi_runtime.hip")).read()
    # one pass with both settings: levels_kernel is launched only where the shading is not
    assert stage.count("if (src.shading) launch_shading(m, src.levels, ") == 2 and stage.count("else if (src.levels) launch_levels(") == 2


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## Frame shading"), ("docs/EXTENSIONS.md", "## Match shading map"), ("README.md", "set_frame_shading"),
                      ("README.md", "shading.hip.h"), ("README.md", "slideo_matcher_shading_begin"), ("README.md", "learn_frame_shading_from_matches"),
                      ("README.md", "match shading map"), ("INTEGRATION.md", "slideo_group_set_frame_shading"),
                      ("INTEGRATION.md", "slideo_matcher_shading_begin")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- slideo_shading_field against the restatement ------------------------------------------------------------------------------------

def _field_both(capi, cnt, sf, sp, cell, min_count, lo, hi, smooth):
    want = R.field(cnt, sf, sp, cell, min_count, lo, hi, smooth)
    cnt, sf, sp = (np.ascontiguousarray(a, np.uint64) for a in (cnt, sf, sp))
    gh, gw = cnt.shape
    out, used = np.full((gh + 1, gw + 1), 7, np.uint16), C.c_int32(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = capi.lib().slideo_shading_field(p(cnt), p(sf), p(sp), gw, gh, cell, C.c_int64(min_count), lo, hi, smooth, p(out), C.byref(used))
    if want is None:
        assert rc == 1 and (out == 7).all() and used.value == -1, "a refusal writes nothing"
        return None
    assert rc == 0 and used.value == want[1]
    assert np.array_equal(out, want[0]), (out, want[0])
    return out


def _sums(gh, gw, ratio_q12, cnt=100, level=300):
    """cnt samples per cell whose page side sums to ratio_q12 / 4096 of the frame side."""
    c = np.full((gh, gw), cnt, np.uint64)
    f = np.full((gh, gw), cnt * level, np.uint64)
    p = (f.astype(object) * ratio_q12 // 4096).astype(np.uint64)
    return c, f, np.minimum(p, 765 * c)


def test_field_named_arrays(capi):
    # one valid cell: the fill carries its value everywhere, whatever the smoothing
    c, f, p = np.zeros((4, 5), np.uint64), np.zeros((4, 5), np.uint64), np.zeros((4, 5), np.uint64)
    c[2, 3], f[2, 3], p[2, 3] = 100, 20000, 30000
    for smooth in (0, 16):
        assert (_field_both(capi, c, f, p, 32, 64, 64, 2048, smooth) == 384).all()
    # a valid row only: every column keeps its own value down the grid
    c[:], f[:], p[:] = 0, 0, 0
    c[1], f[1] = 100, 20000
    p[1] = [10000, 20000, 30000, 40000, 50000]
    g = _field_both(capi, c, f, p, 16, 1, 64, 2048, 0)
    assert (g[:, 0] == 128).all() and (g[:, 5] == 640).all() and (g[:, 1] == 192).all()
    # an island that needs three fill rounds: a 1 x 7 strip valid in the middle
    c, f, p = np.zeros((1, 7), np.uint64), np.zeros((1, 7), np.uint64), np.zeros((1, 7), np.uint64)
    c[0, 3], f[0, 3], p[0, 3] = 64, 6400, 3200
    assert (_field_both(capi, c, f, p, 64, 64, 1, 65535, 0) == 128).all()
    c[0, 3] = 63                                                   # one sample short: no valid cell
    assert _field_both(capi, c, f, p, 64, 64, 1, 65535, 0) is None
    # smooth 0 and 16 on a step, clamps hit on both sides
    c, f, p = _sums(6, 6, 4096)
    p[:, 3:] = np.minimum(f[:, 3:] * np.uint64(40), np.uint64(765) * c[:, 3:])     # gain 2.55 at most: clamped to 2.0 below
    p[:, :1] = 0                                                   # gain 0: clamped up to 0.5
    g0 = _field_both(capi, c, f, p, 32, 1, 128, 512, 0)
    assert g0[0, 0] == 128 and g0[3, 6] == 512 and g0[3, 2] == 256
    g16 = _field_both(capi, c, f, p, 32, 1, 128, 512, 16)
    assert g16.min() > 128 and g16.max() < 512
    # ties in every rounding: r = x.5 rounds up ((2 * 4096 * 1 + 16384) / (2 * 16384) = 0.75 -> 0; 3 / 2 -> 2 in the node mean)
    c, f, p = np.full((1, 2), 100, np.uint64), np.array([[4096, 4096]], np.uint64), np.array([[24, 25]], np.uint64)      # r = 24, 25
    g = _field_both(capi, c, f, p, 16, 1, 1, 65535, 0)
    assert g.tolist() == [[2, 2, 2]] * 2                           # (24 + 8) >> 4 = 2; the mean 24.5 -> 25 -> 2; (25 + 8) >> 4 = 2
    f[:] = 8192; p[0] = [1, 3]                                     # r = (8192 + 8192) / 16384 = 1 (0.5 rounds up), (24576 + 8192) / 16384 = 2
    assert R.field(c, f, p, 16, 1, 1, 65535, 0) is not None
    _field_both(capi, c, f, p, 16, 1, 1, 65535, 0)
    # sums beyond 64 bits in the product: 2^54 samples of 765
    big = np.array([[1 << 54]], dtype=np.uint64)
    g = _field_both(capi, big, big * np.uint64(3), big * np.uint64(765), 32, 1, 1, 65535, 0)
    assert g[0, 0] == 255 * 256


def test_field_random_arrays(capi):
    rng = np.random.default_rng(5)
    for k in range(60):
        cell = R.CELLS[k % 3]
        gh, gw = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        c = rng.integers(0, 200, (gh, gw)).astype(np.uint64)
        c[rng.random((gh, gw)) < 0.4] = 0
        f = (rng.integers(0, 766, (gh, gw)).astype(np.uint64) * c) // np.uint64(1 + k % 3)
        p = (rng.integers(0, 766, (gh, gw)).astype(np.uint64) * c) // np.uint64(1 + k % 2)
        lo, hi = int(rng.integers(1, 257)), int(rng.integers(256, 4000))
        _field_both(capi, c, f, p, cell, int(rng.integers(1, 120)), lo, hi, int(rng.integers(0, 17)))


def test_field_refusals(capi):
    c, f, p = _sums(3, 4, 5000)
    ok = dict(cell=32, min_count=64, lo=64, hi=2048, smooth=1)
    assert _field_both(capi, c, f, p, **ok) is not None
    for change in (dict(min_count=0), dict(lo=0), dict(lo=257), dict(hi=255), dict(hi=65536), dict(smooth=-1), dict(smooth=17), dict(cell=8),
                   dict(cell=48), dict(min_count=101)):
        assert _field_both(capi, c, f, p, **dict(ok, **change)) is None, change
    bad = f.copy(); bad[1, 1] = 765 * 100 + 1
    assert _field_both(capi, c, bad, p, **ok) is None and _field_both(capi, c, f, bad, **ok) is None
    assert _field_both(capi, np.zeros((1, 257), np.uint64), np.zeros((1, 257), np.uint64), np.zeros((1, 257), np.uint64), **dict(ok, cell=16)) is None
    L, out = capi.lib(), np.zeros((4, 5), np.uint16)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.slideo_shading_field(pp(c), pp(f), pp(p), 0, 3, 32, C.c_int64(1), 64, 2048, 0, pp(out), None) == 1
    with pytest.raises(capi.SlideoError):
        capi.shading_field(c, f, p, 32, 0, 64, 2048, 1)
    g, used = capi.shading_field(c, f, p, 32, 64, 64, 2048, 1)
    assert used == 12 and np.array_equal(g, R.field(c, f, p, 32, 64, 64, 2048, 1)[0])


# ---- the apply rule --------------------------------------------------------------------------------------------------------------------

def test_apply_rule_edges():
    rng = np.random.default_rng(3)
    for cell in R.CELLS:
        for aw, ah in ((cell * 2, cell), (1, 1), (cell + 1, cell - 1)):          # an exact multiple of the cell, one pixel, ragged
            img = rng.integers(0, 256, (ah, aw, 3), dtype=np.uint8)
            assert np.array_equal(R.apply(img, cell, R.identity(aw, ah, cell)), img)                         # the identity
            one = R.apply(img, cell, np.ones_like(R.identity(aw, ah, cell)))
            assert np.array_equal(one, (img >= 128).astype(np.uint8))                                        # a gain of 1: 0 or 1
            top = R.apply(img, cell, np.full_like(R.identity(aw, ah, cell), 65535))
            assert np.array_equal(top, np.where(img == 0, 0, 255))                                           # saturation at 65535
            gw, gh = R.grid(aw, ah, cell)
            assert R.identity(aw, ah, cell).shape == (gh + 1, gw + 1) and gw == -(-aw // cell)
    # bilinear between the nodes: the gain at a node is the node's, half-way it is the mean
    g = np.array([[256, 512], [256, 512]], np.uint16)
    G = R.gain_map(16, 16, 16, g)
    assert G[0, 0] == 256 and G[5, 8] == 384 and G[15, 15] == 256 + 240


# ---- tools/shading_hostcheck.cpp -----------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "shading_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("shading"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("shading_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _apply_case(exe, tmp, w, h, stride, n, sofs, dofs, in_place, seed, cell, gains, lut):
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, (n, h, stride), dtype=np.uint8)
    imgs = np.ascontiguousarray(buf[:, :, :3 * w]).reshape(n, h, w, 3)
    cin, cout = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(cin, "wb") as f:
        f.write(struct.pack("<10i", w, h, n, stride, stride, sofs, dofs, 1 if in_place else 0, cell, 0 if lut is None else 1))
        f.write(np.ascontiguousarray(LR.identity() if lut is None else lut, np.uint8).tobytes())
        f.write(np.ascontiguousarray(gains, np.uint16).tobytes())
        f.write(buf.tobytes())
    flags = subprocess.check_output([exe, "apply", cin, cout]).decode()
    got = np.fromfile(cout, np.uint8)
    # the whole destination buffer: the shaded pixels, and between the rows the source's own bytes (in place) or the fill that was
    # there (out of place: never written)
    want = buf.copy() if in_place else np.full_like(buf, 0xAA)
    shaded = R.apply(imgs, cell, gains)
    want[:, :, :3 * w] = (shaded if lut is None else LR.apply(shaded, lut)).reshape(n, h, 3 * w)
    assert got.size == (n * h - 1) * stride + 3 * w
    assert np.array_equal(got, want.reshape(-1)[:got.size]), (w, h, stride, sofs, in_place, cell, flags)
    assert "rule 1" in flags
    if not in_place:
        assert "src_unchanged 1" in flags
    return flags


def _fields(w, h, cell, k):
    return [R.random_field(w, h, cell, k), R.ramp_field(w, h, cell), R.random_field(w, h, cell, k, 200, 400)][k % 3]


def test_host_build_of_shading_thread_equals_the_restatement(hostcheck, tmp_path):
    """Every size, stride and cell, in place and out of place, with and without the table, two frames: both loads and both stores
    were taken on either side."""
    seen = set()
    lut = LR.random_lut(3)
    k = 0
    for w, h in R.SIZES:
        for stride in R.strides(w):
            for cell in R.CELLS if w * h < 100000 else (R.CELLS[k % 3],):
                for in_place in (True, False):
                    for sofs, dofs in ((0, 0), (4, 1)):
                        k += 1
                        table = (k + k // 4) % 2                  # (every pair of place and offsets meets both instances)
                        flags = _apply_case(hostcheck, tmp_path, w, h, stride, 2, sofs, dofs, in_place, k, cell, _fields(w, h, cell, k),
                                            lut if table else None)
                        seen.update((in_place, "lut %d" % table, word) for word in re.findall(r"(?:in4|out4) \d", flags))
    for place in (True, False):
        for table in ("lut 0", "lut 1"):
            for word in ("in4 0", "in4 1", "out4 0", "out4 1"):
                assert (place, table, word) in seen, (place, table, word)


def test_sanitized_host_build_of_shading_thread(hostcheck_san, tmp_path):
    """Base offsets 0, 1, 2, 4 and 8 on exact-size heap buffers (the gains too), in place and out of place, with and without the
    table: a dword access at an address that is not a multiple of 4, a load past the last pixel, a node outside the field or a store
    outside the image would be reported.  Run as a program: nothing is preloaded."""
    lut = LR.random_lut(4)
    seen = set()
    for k, (w, h) in enumerate(R.SIZES):
        big = w * h > 100000
        for j, stride in enumerate(R.strides(w)):
            for i, ofs in enumerate((0, 1, 2, 4, 8)):
                if big and (i + j) % 3:
                    continue                                      # (the large size: every offset and stride once, not every pair)
                cell = R.CELLS[(i + j + k) % 3]
                for in_place in (True, False):
                    for table in (None, lut):
                        flags = _apply_case(hostcheck_san, tmp_path, w, h, stride, 1 + (k + i) % 2, ofs, (0, ofs)[(i + j) % 2], in_place, 100 + k, cell,
                                            _fields(w, h, cell, i + j), table)
                        seen.update(re.findall(r"(?:in4|out4) \d", flags))
    assert seen == {"in4 0", "in4 1", "out4 0", "out4 1"}


def test_apply_rule_edges_through_the_sanitized_host_build(hostcheck_san, tmp_path):
    """The edges of test_apply_rule_edges through the kernel's thread body and the header's plain rule (frame_settings.h
    frame_shading_pixel, the check's `rule 1`): the identity, a gain of 1, saturation at 65535, a width that is an exact multiple of
    the cell, one pixel."""
    k = 0
    for cell in R.CELLS:
        for aw, ah in ((cell * 2, cell), (1, 1), (cell + 1, cell - 1)):
            for gains in (R.identity(aw, ah, cell), np.ones_like(R.identity(aw, ah, cell)), np.full_like(R.identity(aw, ah, cell), 65535)):
                for lut in (None, LR.random_lut(5)):
                    k += 1
                    _apply_case(hostcheck_san, tmp_path, aw, ah, 3 * aw + k % 2, 1, k % 3, 0, bool(k % 2), k, cell, gains, lut)


# ---- the session's per-frame body (hostcheck session) ----------------------------------------------------------------------------------

def _host_sums(exe, tmp, unit_args, cell, tile_rows=None):
    unit, out = str(tmp / "unit.bin"), str(tmp / "out.bin")
    TA._write_unit(unit, *unit_args)
    stats = subprocess.check_output([exe, "session", unit, out, str(cell)] + ([str(tile_rows)] if tile_rows else [])).decode().split()
    got = np.fromfile(out, np.uint64)
    ah, aw = unit_args[1][0]["image"].shape[:2]
    gw, gh = R.grid(aw, ah, cell)
    assert got.size == 3 * gw * gh + 1
    return got[:-1].reshape(3, gh, gw), int(got[-1]), dict(zip(stats[::2], map(int, stats[1::2])))


def _check_session_cases(oracle, exe, tmp, cells):
    for i, (name, fa, pset, min_inliers, min_hits, flats) in enumerate(T.constructed_cases()):
        cfg, frames, tp, pxy, pages = TA._oracle_unit(oracle, name, fa, pset)
        for flat in sorted(set(flats) | {0, 8, 255}):
            for cell in cells if flat == 255 else (cells[(i + flat) % len(cells)],):
                want = R.sums(frames, cell, min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=cfg.verify_model, thr=cfg.ransac_threshold,
                              train_page=tp, page_xy=pxy, pages=pages)                     # (asserts the guard on every tested value)
                args = (cfg, frames, tp, pxy, pages, min_inliers, min_hits, flat)
                got, counted, hs = _host_sums(exe, tmp, args, cell)
                assert np.array_equal(got, want[0]) and counted == want[2], (name, flat, cell)
                assert hs["tiles"] <= 1 and hs["samples"] == int(want[0][0].sum())
                if name in ("T2-inliers", "T2-hits"):
                    assert counted == 0 and not got.any()
                elif flat == 255:
                    # a thread adds when its cell changes, not per sample: tens of pixels share a cell
                    assert counted >= 1 and hs["samples"] > 0 and hs["adds"] * 2 < hs["samples"] * 3, hs
                # the same through row tiles of 7 rows: the zeroing, the flush and the seam between tiles
                got7, counted7, hs7 = _host_sums(exe, tmp, args, cell, tile_rows=7)
                assert np.array_equal(got7, got) and counted7 == counted and (counted == 0 or hs7["tiles"] > 10), (name, flat, cell)
    # a unit whose run raised a re-run bit counts nothing
    name, fa, pset, mi, mh, flats = T.constructed_cases()[0]
    cfg, frames, tp, pxy, pages = TA._oracle_unit(oracle, name, fa, pset)
    for flags, mask, counts in ((4, 12, False), (8, 12, False), (8, 4, True), (2, 12, True)):
        got, counted, _ = _host_sums(exe, tmp, (cfg, frames, tp, pxy, pages, mi, mh, 255, flags, mask), 32)
        assert bool(got.sum()) == counts and bool(counted) == counts, (flags, mask)


def test_host_build_of_the_session_body_equals_the_restatement(oracle, hostcheck, tmp_path):
    _check_session_cases(oracle, hostcheck, tmp_path, R.CELLS)


def test_sanitized_host_build_of_the_session_body(oracle, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks with every array — the bins [3][cells] and the accumulators among them — in an
    allocation of exactly its size.  A stand-alone program: nothing is loaded into Python."""
    _check_session_cases(oracle, hostcheck_san, tmp_path, R.CELLS)


def test_wild_features_reach_no_cell(oracle, hostcheck_san, tmp_path):
    """A caller's own features may hold any float: keypoints and a transform that send samples to negative, huge, infinite or NaN
    positions count nowhere and read nothing outside the frame or the bins (the sanitized build), whole and in row tiles of 7 rows."""
    name, fa, pset, mi, mh, flats = T.constructed_cases()[0]
    cfg, frames, tp, pxy, pages = TA._oracle_unit(oracle, name, fa, pset)
    slot = T.contributor(frames[0]["cands"], 0)
    kw = dict(min_inliers=mi, min_hits=1, flat=255, model=cfg.verify_model, thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy, pages=pages, guard=False)
    for k, wild in enumerate(([1e300, 0, 0, 0, 1e300, 0], [np.nan] * 6, [np.inf, 0, 5, 0, -np.inf, 5], [1, 0, -1e9, 0, 1, 2.0 ** 40], [0, 0, 639.4, 0, 0, 359.4])):
        f = dict(frames[0])
        f["cands"] = list(f["cands"])
        M = np.array(f["cands"][slot][2], np.float64, copy=True)
        M[:6] = wild
        f["cands"][slot] = (f["cands"][slot][0], f["cands"][slot][1], M)
        for cell in R.CELLS:
            want = R.sums([f], cell, **kw)
            got, counted, _ = _host_sums(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, pages, mi, 1, 255), cell, tile_rows=(None, 7)[k % 2])
            assert np.array_equal(got, want[0]) and counted == want[2], (k, cell)
    # keypoints moved wildly under the true transform: the hits are the untouched ones, and the samples stay inside the frame
    f = dict(frames[0]); f["xy"] = np.array(f["xy"], np.float32, copy=True)
    f["xy"][:6] = [[-0.5, 10], [10, -3e9], [1e30, 10], [10, 360], [np.nan, 10], [np.inf, -np.inf]]
    want = R.sums([f], 16, **kw)
    got, counted, _ = _host_sums(hostcheck_san, tmp_path, (cfg, [f], tp, pxy, pages, mi, 1, 255), 16)
    assert np.array_equal(got, want[0]) and counted == want[2] == 1
    assert got[0].sum() > 0


# ---- the use -------------------------------------------------------------------------------------------------------------------------

def test_the_use_scene_meets_its_conditions_on_the_cpu(capi, oracle, synth):
    """The canvas scene of the evidence map (tests/evidence_ref.py canvas_scene: a 640x360 window in a 960x540 textured canvas, 4 pages,
    16 frames, ORB-3000, min_rating 12) with the window alone under a radial falloff that reaches 0.2 in its corners
    (shading_ref.window_falloff, a = 0.8), through the CPU restatement of the pipeline, evidence_ref.votes_of, tone_ref's sampler and
    shading_ref, at cell 32, min_inliers 20, min_hits 20, flat 255; min_count 64, gains clamped to 64..2048, smooth 1:
      - without a field at most 8 of 16 pages are right;
      - at least 8 frames contribute;
      - under the learnt field all 16 are right with every similarity at least 0.70;
      - a tone table then learnt on the shaded frames (tone_ref.USE) keeps all 16;
      - a field learnt from the clean frames changes no verdict of the clean frames.
    The library's slideo_shading_field gives the restatement's field on these sums.
    Found, not gated (printed; docs/EXTENSIONS.md "Match shading map" holds the figures): the tone table alone on the unshaded
    falloff frames, and the field's node error against 1 / falloff."""
    pages, frames, truth = E.canvas_scene(synth)
    U, TU = R.USE, T.USE
    cfg = small_cfg(oracle, nfeatures=E.SCENE["nfeatures"], min_rating=U["min_rating"])
    db = oracle.PageDB(cfg)
    db.add_pages(pages, threads=4)
    assert db.finalize() == 0
    train = db.train()
    tp, pxy = E.deck_of(db, len(pages))
    page_recs = {p: (pages[p].shape[1], pages[p].shape[0], oracle.small_image(pages[p], cfg.small_area)) for p in range(len(pages))}

    def records(fr):
        recs = []
        for f in fr:
            _, cands = db.match_frame_trace(f)
            kp, desc = oracle.orb(f, cfg)
            recs.append(T.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, cands, train, f))
        return recs

    def learn_field(recs):
        sums, through, counted = R.sums(recs, U["cell"], min_inliers=U["min_inliers"], min_hits=U["min_hits"], flat=U["flat"], model=0,
                                        thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy, pages=page_recs, guard=False)
        got = R.field(sums[0], sums[1], sums[2], U["cell"], U["min_count"], U["min_gain"], U["max_gain"], U["smooth"])
        assert got is not None
        lib, used = capi.shading_field(sums[0], sums[1], sums[2], U["cell"], U["min_count"], U["min_gain"], U["max_gain"], U["smooth"])
        assert np.array_equal(lib, got[0]) and used == got[1]
        return got[0], counted, got[1]

    def learn_table(recs):
        cnt, sm, _, _ = T.counts(recs, min_inliers=TU["min_inliers"], min_hits=TU["min_hits"], flat=TU["flat"], model=0, thr=cfg.ransac_threshold,
                                 train_page=tp, page_xy=pxy, pages=page_recs, guard=False)
        return T.lut(cnt, sm, TU["min_count"])

    right = lambda v: int((v["page_idx"] == truth).sum())
    sims = lambda v: (float(v["similarity"][v["page_idx"] == truth].min()), float(np.median(v["similarity"][v["page_idx"] == truth])))
    cell = U["cell"]
    dim = R.window_falloff(frames)
    v_clean = db.match_frames(frames, threads=8)
    v_dim = db.match_frames(dim, threads=8)
    dim_recs = records(dim)
    gains, counted, used = learn_field(dim_recs)
    shaded = R.apply(dim, cell, gains)
    v_field = db.match_frames(shaded, threads=8)
    lut = learn_table(records(shaded))
    v_both = db.match_frames(LR.apply(shaded, lut), threads=8)
    tone_alone = learn_table(dim_recs)
    v_tone = db.match_frames(LR.apply(dim, tone_alone), threads=8) if tone_alone is not None else None
    cgains, _, _ = learn_field(records(frames))
    v_cfield = db.match_frames(R.apply(frames, cell, cgains), threads=8)
    # the field's node error against 1 / falloff, over the nodes inside the window
    H, W = frames.shape[1:3]
    j, i = np.mgrid[0:gains.shape[0], 0:gains.shape[1]]
    x, y = np.minimum(i * cell, W - 1) - E.WIN_X, np.minimum(j * cell, H - 1) - E.WIN_Y
    inside = (x >= 0) & (x < E.WIN_W) & (y >= 0) & (y < E.WIN_H)
    rho2 = (((x - (E.WIN_W - 1) / 2) / (E.WIN_W / 2)) ** 2 + ((y - (E.WIN_H - 1) / 2) / (E.WIN_H / 2)) ** 2) / 2
    err = (gains / 256.0) * (1 - U["a"] * rho2) - 1
    print("the use on the CPU: clean %d of 16 (similarity min %.3f median %.3f); falloff %d (%.3f / %.3f); field %d (%.3f / %.3f); field + table %d "
          "(%.3f / %.3f); table alone %s; %d frames contributed, %d cells used; node error against 1 / falloff inside the window: median %+.3f, "
          "worst %+.3f; clean field gains %.2f..%.2f, %d of 16"
          % (right(v_clean), *sims(v_clean), right(v_dim), *sims(v_dim), right(v_field), *sims(v_field), right(v_both), *sims(v_both),
             "none" if v_tone is None else "%d (%.3f / %.3f)" % ((right(v_tone),) + sims(v_tone)), counted, used, float(np.median(err[inside])),
             float(err[inside][np.argmax(np.abs(err[inside]))]), cgains.min() / 256, cgains.max() / 256, right(v_cfield)))
    assert right(v_dim) <= 8
    assert counted >= 8
    assert right(v_field) == 16 and float(v_field["similarity"].min()) >= 0.70
    assert right(v_both) == 16
    assert np.array_equal(v_cfield["page_idx"], v_clean["page_idx"]) and right(v_clean) == 16
