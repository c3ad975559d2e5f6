"""YUV transfer (include/slideo_amd.h "YUV transfer") without a GPU: the header, the exports and the docs; the library's tables
held to the header's formulas in float64; the round trip of the forward model through the restatement; the setter's rules (through
tools/yuv_transfer_hostcheck.cpp, a stand-alone program over csrc/frame_settings.h); and the kernel's per-thread body compiled for
the host — with and without -fsanitize=address,undefined — against tests/yuv_transfer_ref.py over the matrix of the GPU test."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import yuv_transfer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slideo_amd.h")
NEW = ["slideo_matcher_set_yuv_transfer", "slideo_matcher_yuv_transfer", "slideo_group_set_yuv_transfer", "slideo_yuv_transfer_tables"]
VALUES = (("SDR", 0), ("HLG", 1), ("PQ", 2))
CASES = [(t, r, n) for t in (R.HLG, R.PQ) for r in (R.LIMITED, R.FULL) for n in R.NITS]


# ---- header, exports, null handles, docs ------------------------------------------------------------------------------------------------

def test_header_declares_the_calls_and_constants():
    h = open(HDR).read()
    for name in NEW:
        assert re.search(r"int32_t\s+%s\(" % name, h), name
    for name, v in VALUES:
        assert re.search(r"#define SLIDEO_YUV_TRANSFER_%s\s+%d\b" % (name, v), h), name
    assert "#define SLIDEO_ABI_VERSION 7" in h
    assert not re.search(r"#define SLIDEO_YUV_MATRIX_\w+\s+2\b", h)           # no third matrix value
    sec = h.split("---- YUV transfer", 1)[1].split("/* ----", 1)[0]
    for word in ("DEPARTURE", "Contract", "THE LIBRARY'S TABLES ARE THE DEFINITION", "MATRIX IS NOT CONSULTED", "SHIFT = 18", "0.2627", "0.0593",
                 "16383", "ST 2084", "0.17883277", "0.28466892", "0.55991073", "1 << 13", "(o + 2) >> 2", "BGR calls never", "Out of scope",
                 "bilinear chroma under a transfer", "SLIDEO_YUV_DEPTH_8", "203"):
        assert word in sec, word
    for v in R.COEF_LIMITED[:5] + R.COEF_FULL[:5] + tuple(x for row in R.GAMUT for x in row):
        assert str(v) in sec, v
    # the sampling section's out-of-scope lists are not touched
    samp = h.split("---- YUV sampling", 1)[1].split("/* ----", 1)[0]
    assert "packed 10-bit (Y210, v210); 4:1:1 and 4:4:0" in samp


def test_library_exports_them_at_abi_7(capi):
    L = capi.lib()
    assert L.slideo_abi_version() == 7
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert C.sizeof(capi.Yuv420Layout) == 32 and C.sizeof(capi.Config) == 168


def test_null_handles_and_outputs(capi):
    L = capi.lib()
    t, n = C.c_int32(), C.c_float()
    assert L.slideo_matcher_set_yuv_transfer(None, 0, 0.0) == 1
    assert L.slideo_group_set_yuv_transfer(None, 1, 0.0) == 1
    assert L.slideo_matcher_yuv_transfer(None, C.byref(t), C.byref(n)) == 1
    # any output may be null; a bad enumeration value or bad nits is INVALID_ARG, and SDR has no tables
    assert L.slideo_yuv_transfer_tables(1, 0, 0.0, None, None, None, None) == 0
    coef = (C.c_int32 * 7)()
    assert L.slideo_yuv_transfer_tables(2, 1, 100.0, coef, None, None, None) == 0 and tuple(coef) == R.COEF_FULL
    for tr, rg, nt in ((0, 0, 0.0), (3, 0, 0.0), (-1, 0, 0.0), (1, 2, 0.0), (1, -1, 0.0), (1, 0, 0.5), (1, 0, 20000.0), (2, 0, float("nan")),
                       (2, 0, float("inf")), (2, 0, -1.0)):
        assert L.slideo_yuv_transfer_tables(tr, rg, nt, coef, None, None, None) == 1, (tr, rg, nt)


def test_names_and_python_value_errors(capi):
    assert capi.YUV_TRANSFERS == {"sdr": 0, "hlg": 1, "pq": 2}
    assert [capi.yuv_transfer_value(n) for n in ("sdr", "HLG", "Pq", 2, np.int32(1))] == [0, 1, 2, 2, 1]
    for bad in ("hdr10", "smpte2084", "", None, 1.5, True, (1,)):
        with pytest.raises(ValueError):
            capi.yuv_transfer_value(bad)
    with pytest.raises(ValueError):
        capi.yuv_transfer_tables("hlg", "studio")
    with pytest.raises(capi.SlideoError):
        capi.yuv_transfer_tables("sdr")
    with pytest.raises(capi.SlideoError):
        capi.yuv_transfer_tables(7)


def test_mirrors_carry_the_option(capi):
    from slideo_amd import matching as mt
    assert mt.HipImageVideoMatcher(yuv_transfer=("hlg", 203))._yuv_transfer == ("hlg", 203)
    assert mt.HipImageVideoMatcher(yuv_transfer="pq")._yuv_transfer == ("pq", 0)
    assert mt.HipImageVideoMatcher()._yuv_transfer is None
    for cls in (capi.Matcher, capi.Group):
        assert hasattr(cls, "set_yuv_transfer") and hasattr(cls, "yuv_transfer")
    hpp = open(os.path.join(ROOT, "slideo_amd", "host", "matching.hpp")).read()
    assert "with_yuv_transfer" in hpp and "slideo_group_set_yuv_transfer" in hpp
    rs = open(os.path.join(ROOT, "crates", "matching-hip", "src", "lib.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    assert "yuv_transfer" in rs and "slideo_group_set_yuv_transfer" in rs
    for name in NEW:
        assert "pub fn %s(" % name in ffi, name
    for name, v in VALUES:
        assert re.search(r"pub const SLIDEO_YUV_TRANSFER_%s: i32 = %d;" % (name, v), ffi), name


def test_docs_name_the_feature():
    for f, needle in (("docs/EXTENSIONS.md", "## YUV transfer"), ("README.md", "set_yuv_transfer"), ("INTEGRATION.md", "slideo_group_set_yuv_transfer"),
                      ("README.md", "yuv_transfer.hip.h"), ("README.md", "YUV transfer")):
        assert needle in open(os.path.join(ROOT, f)).read(), (f, needle)


# ---- the tables against the header's formulas --------------------------------------------------------------------------------------------

def _held_to(got, formula, what):
    """Every entry within 1 of the formula's rounded value, and equal to it wherever the unrounded value is further than 1e-6 from
    a half-integer."""
    got, formula = np.asarray(got, np.int64), np.asarray(formula, np.float64)
    want = np.rint(formula).astype(np.int64)
    assert np.all(np.abs(got - want) <= 1), (what, np.argwhere(np.abs(got - want) > 1)[:4])
    clear = np.abs(np.abs(formula - np.floor(formula)) - 0.5) > 1e-6
    assert np.array_equal(got[clear], want[clear]), (what, np.argwhere((got != want) & clear)[:4])


@pytest.mark.parametrize("transfer,rng,nits", CASES, ids=lambda v: str(v))
def test_tables_against_the_formulas(capi, transfer, rng, nits):
    T = R.tables(capi, transfer, rng, nits)
    coef = R.COEF_FULL if rng == R.FULL else R.COEF_LIMITED
    assert tuple(T.coef) == coef
    _held_to(T.coef[:5], R.coef_formula(rng)[:5], "coef")
    assert R.coef_formula(rng)[5:] == coef[5:]
    # gamut: off the diagonal the rounded G 2^14, the diagonal what makes the row sum 2^14
    G = R.gamut_float() * 16384.0
    off = ~np.eye(3, dtype=bool)
    _held_to(T.gamut[off], G[off], "gamut")
    assert np.all(T.gamut.sum(axis=1) == 16384)
    assert np.all(np.abs(T.gamut[~off] - G[~off]) <= 2)
    assert tuple(map(tuple, T.gamut.tolist())) == R.GAMUT
    _held_to(T.lin, R.lin_formula(transfer, nits), "LIN")
    _held_to(T.out, R.out_formula(), "OUT")
    assert np.all(np.diff(T.lin) >= 0) and np.all(np.diff(T.out) >= 0) and np.all(np.diff(T.out) <= 1)
    assert T.lin[0] == 0 and T.lin[1023] == 16383 and T.out[0] == 0 and T.out[4095] == 255
    assert T.lin.shape == (1024,) and T.out.shape == (4096,)
    # the int32 and 24-bit bounds of the header, recomputed from these integers
    CY, CUB, CUG, CVG, CVR, yofs, shift = T.coef
    assert shift == 18
    lim24 = 1 << 23
    assert max(abs(c) for c in T.coef[:5]) < lim24 and np.abs(T.gamut).max() < lim24 and T.lin.max() <= 16383 < lim24
    ymax = (1023 - yofs) * CY
    products = [ymax, 512 * abs(CUB), 512 * abs(CUG), 512 * abs(CVG), 512 * abs(CVR)]
    assert max(products) <= 2.94e8
    sums = [ymax + (1 << 17) + 511 * max(CUB, CVR), ymax + (1 << 17) + 512 * (abs(CUG) + abs(CVG)), (1 << 17) - 512 * max(CUB, CVR),
            (1 << 17) - 511 * (abs(CUG) + abs(CVG))]
    assert max(abs(s) for s in sums) <= 5.82e8 < 2 ** 31
    assert np.abs(T.gamut).max() * 16383 <= 4.46e8
    pos, neg = np.where(T.gamut > 0, T.gamut, 0).sum(axis=1), np.where(T.gamut < 0, T.gamut, 0).sum(axis=1)
    assert pos.max() * 16383 + (1 << 13) < 2 ** 31 and neg.min() * 16383 > -2 ** 31


def test_tables_do_not_depend_on_what_they_should_not(capi):
    a, b = R.tables(capi, R.HLG, R.LIMITED, 0), R.tables(capi, R.HLG, R.FULL, 203)
    assert np.array_equal(a.lin, b.lin) and np.array_equal(a.out, b.out) and np.array_equal(a.gamut, b.gamut)      # 0 means 203
    c = R.tables(capi, R.PQ, R.LIMITED, 0)
    assert not np.array_equal(a.lin, c.lin) and np.array_equal(a.out, c.out) and a.coef == c.coef


# ---- the round trip ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transfer,rng,nits", [(t, r, n) for t in (R.HLG, R.PQ) for r in (R.LIMITED, R.FULL) for n in (100, 203)], ids=lambda v: str(v))
def test_round_trip_of_the_forward_model(capi, transfer, rng, nits):
    """frames_to_yuv, then the restatement, at 4:4:4: the 256 greys are within 2 and the median absolute error of seeded random
    colours is at most 1 (the reference alone: greys within 1, median 0, mean 0.23-0.63, p99 3-5)."""
    T = R.tables(capi, transfer, rng, nits)
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    rnd = np.random.default_rng(11).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for img, what in ((grey, "grey"), (rnd, "random")):
        h, w = img.shape[:2]
        for depth in R.DEPTHS:
            L, fb = R.S.make_layout(capi, "i444", w, h, 2)
            yuv = R.frames_to_yuv(img[None], L, fb, transfer, rng, depth, R.S444, nits)
            back = R.to_bgr(yuv[0], w, h, L, T, depth, R.S444)
            err = np.abs(back.astype(np.int64) - img.astype(np.int64))
            print(what, transfer, rng, nits, depth, "max", err.max(), "median", np.median(err), "mean", err.mean(), "p99", np.percentile(err, 99))
            if what == "grey":
                assert err.max() <= 2
            else:
                assert np.median(err) <= 1


def test_read_as_sdr_a_white_page_is_grey(capi):
    """The defect the transfer repairs, on the forward model: an HDR white read under ("bt709", "limited", "10_msb") is far from 255."""
    import yuv_desc_ref as D
    white = np.full((2, 2, 3), 255, np.uint8)
    L, fb = capi.yuv420_layout("nv12", 2, 2, bytes_per_sample=2)
    for transfer, lo, hi in ((R.HLG, 180, 200), (R.PQ, 140, 156)):
        yuv = R.frames_to_yuv(white[None], L, fb, transfer, R.LIMITED, R.D10_MSB, R.S420, 203)
        sdr = D.to_bgr(yuv[0], 2, 2, L, (D.BT709, D.LIMITED, D.D10_MSB))
        assert lo <= int(sdr.min()) and int(sdr.max()) <= hi, (transfer, sdr.min(), sdr.max())
        assert np.all(R.to_bgr(yuv[0], 2, 2, L, R.tables(capi, transfer, R.LIMITED, 203), R.D10_MSB, R.S420) >= 254)


# ---- tools/yuv_transfer_hostcheck.cpp ------------------------------------------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "slideo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "yuv_transfer_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostcheck(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_transfer"), "hostcheck", [])


@pytest.fixture(scope="module")
def hostcheck_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("yuv_transfer_san"), "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _lines(exe, *args):
    out = subprocess.check_output([exe] + [str(a) for a in args]).decode().strip().split("\n")
    return [(int(l.partition(" ")[0]), l.partition(" ")[2]) if not l.startswith("state") else tuple(float(x) for x in l.split()[1:]) for l in out]


def test_host_table_rule_is_the_library_s(capi, hostcheck):
    for transfer, rng, nits in CASES:
        lines = subprocess.check_output([hostcheck, "tables", str(transfer), str(rng), str(nits)]).decode().strip().split("\n")
        T = R.tables(capi, transfer, rng, nits)
        assert lines[0] == "0"
        got = [[int(x) for x in l.split()] for l in lines[1:]]
        assert got[0] == T.coef and got[1] == T.gamut.reshape(-1).tolist() and got[2] == T.lin.tolist() and got[3] == T.out.tolist()
    assert subprocess.check_output([hostcheck, "tables", "0", "0", "0"]).decode().split()[0] == "1"


P010 = ("d", 1, 0, 1)            # ("bt709", "limited", "10_msb"): a 10-bit depth, which a transfer needs


def test_setter_refusals_and_the_state_each_leaves(hostcheck):
    # state: matrix range depth sampling filter transfer white_nits
    assert _lines(hostcheck, "set", *P010, "t", 1, 0) == [(0, "ok"), (0, "ok"), (1, 0, 1, 0, 0, 1, 203)]
    assert _lines(hostcheck, "set", *P010, "t", 2, 100)[-1] == (1, 0, 1, 0, 0, 2, 100)
    assert _lines(hostcheck, "set", *P010, "t", 2, 100, "t", 0, 0)[-1] == (1, 0, 1, 0, 0, 0, 0)
    for lo_hi in (1, 10000):
        assert _lines(hostcheck, "set", *P010, "t", 1, lo_hi)[-1] == (1, 0, 1, 0, 0, 1, lo_hi)
    # bad enumeration values and bad nits: INVALID_ARG, the rule named, the state before stays
    for bad, nits, word in ((3, 0, "none of"), (-1, 0, "none of"), (1, "nan", "white_nits"), (1, 0.5, "white_nits"), (2, 20000, "white_nits"),
                            (1, "inf", "white_nits"), (2, -5, "white_nits"), (0, 203, "must be 0")):
        (code, msg), state = _lines(hostcheck, "set", *P010, "t", 2, 100, "t", bad, nits)[2:]
        assert code == 1 and "yuv transfer" in msg and word in msg, (bad, nits, msg)
        assert state == (1, 0, 1, 0, 0, 2, 100)
    # a transfer with 8-bit samples: both orders are UNSUPPORTED and the values before stay
    a = _lines(hostcheck, "set", "t", 1, 0)
    assert a[0][0] == 5 and "SLIDEO_YUV_DEPTH_8" in a[0][1] and a[1] == (0, 0, 0, 0, 0, 0, 0)
    a = _lines(hostcheck, "set", *P010, "t", 1, 0, "d", 1, 0, 0)
    assert a[2][0] == 5 and "SLIDEO_YUV_DEPTH_8" in a[2][1] and a[3] == (1, 0, 1, 0, 0, 1, 203)
    # which also excludes 422_PACKED, whichever way round
    a = _lines(hostcheck, "set", "s", 3, "t", 1, 0)
    assert a[1][0] == 5 and a[2] == (0, 0, 0, 3, 0, 0, 0)
    a = _lines(hostcheck, "set", *P010, "t", 1, 0, "s", 3)
    assert a[2][0] == 5 and a[3] == (1, 0, 1, 0, 0, 1, 203)
    # a transfer with bilinear chroma while the sampling is not 4:4:4: each of the three set calls that would complete it is refused
    a = _lines(hostcheck, "set", *P010, "c", 1, "t", 1, 0)
    assert a[2][0] == 5 and "out of scope" in a[2][1] and a[3] == (1, 0, 1, 0, 1, 0, 0)
    a = _lines(hostcheck, "set", *P010, "t", 2, 0, "c", 2)
    assert a[2][0] == 5 and "out of scope" in a[2][1] and a[3] == (1, 0, 1, 0, 0, 2, 203)
    a = _lines(hostcheck, "set", *P010, "s", 2, "c", 3, "t", 1, 0, "s", 1)
    assert [x[0] for x in a[:4]] == [0, 0, 0, 0] and a[4][0] == 5 and "out of scope" in a[4][1] and a[5] == (1, 0, 1, 2, 3, 1, 203)
    # the description's, the sampling's and the chroma filter's setters leave the transfer alone
    assert _lines(hostcheck, "set", *P010, "t", 1, 400, "d", 0, 1, 2, "s", 1, "c", 0)[-1] == (0, 1, 2, 1, 0, 1, 400)
    # a refused description or sampling leaves everything, the transfer included
    assert _lines(hostcheck, "set", *P010, "t", 2, 0, "d", 2, 0, 1, "s", 9)[-1] == (1, 0, 1, 0, 0, 2, 203)


def _write_cases(capi, path, shift, n_of):
    """The GPU test's whole matrix as one case file; returns [(frames, w, h, L, tables, depth, sampling, tag)]."""
    want, tabs = [], {}
    with open(path, "wb") as f:
        for k, (s, depth, fmt, name, L, fb, w, h) in enumerate(R.tap_cases(capi)):
            transfer, rng, nits = R.pick(k + shift)
            if (transfer, rng, nits) not in tabs:
                tabs[(transfer, rng, nits)] = R.tables(capi, transfer, rng, nits)
            n = n_of(k)
            frames = [R.random_frame(w, h, L, fb, depth, s, 3 * k + i) for i in range(n)]
            if k % 2 == 0:
                frames[-1] = R.special_frame(w, h, L, fb, depth, s)
            frames = np.stack(frames)
            nbits = struct.unpack("<i", struct.pack("<f", float(nits)))[0]
            f.write(struct.pack("<12i3q", w, h, n, transfer, rng, depth, s, L.y_stride, L.uv_stride, L.uv_step, nbits, frames.size, L.u_offset, L.v_offset, fb))
            f.write(frames.tobytes())
            want.append((frames, w, h, L, tabs[(transfer, rng, nits)], depth, s, (fmt, name, transfer, rng, nits)))
    return want


def _check(exe, capi, tmp, shift, n_of):
    cin, cout = str(tmp / "cases.bin"), str(tmp / "out.bin")
    want = _write_cases(capi, cin, shift, n_of)
    text = subprocess.check_output([exe, "convert", cin, cout]).decode()
    hits = {k: int(v) for k, v in (l.split() for l in text.strip().split("\n"))}
    assert hits["records"] == len(want)
    got = np.fromfile(cout, np.uint8)
    at = 0
    for frames, w, h, L, T, depth, s, tag in want:
        for fr in frames:
            img = got[at:at + w * h * 3].reshape(h, w, 3)
            at += w * h * 3
            ref = R.to_bgr(fr, w, h, L, T, depth, s)
            assert np.array_equal(img, ref), (tag, w, h, depth, s, np.argwhere(img != ref)[:4])
    assert at == got.size
    return hits


PATHS = ("y8", "y4", "y_bytes", "c8", "c4", "c_bytes", "out4", "out_bytes")


def test_host_build_of_the_kernel_body_equals_the_restatement(capi, hostcheck, tmp_path):
    """The whole matrix, two frames each, the transfer, the range and white_nits rotating; every record at five source offsets.
    Every wide load, every fallback and both store paths were taken."""
    hits = _check(hostcheck, capi, tmp_path, 0, lambda k: 2)
    for p in PATHS:
        assert hits[p] > 0, (p, hits)


def test_sanitized_host_build_over_the_whole_matrix(capi, hostcheck_san, tmp_path):
    """Address and undefined-behaviour checks on exact-size buffers and exact-size tables at source offsets 0, 1, 2, 4 and 8: a wide
    load at an address that is not a multiple of its size, a load past the last sample, a table index past its end or a store past
    the image would be reported.  A stand-alone program: nothing is loaded into Python."""
    hits = _check(hostcheck_san, capi, tmp_path, 5, lambda k: 1 + k % 2)
    for p in PATHS:
        assert hits[p] > 0, (p, hits)
