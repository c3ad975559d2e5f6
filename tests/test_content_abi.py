"""Frame content box on a CPU-only box (include/slideo_amd.h "Frame content box"): the header declares the five calls, the library
exports them at ABI 7 with their ctypes signatures and an unchanged slideo_config, every call refuses a null handle, the Python
methods, learn_frame_region and the Rust declarations exist; the numpy restatement (tests/content_ref.py) on hand-computed cases;
and the kernels' per-thread bodies (csrc/content.hip.h), compiled for the host plain and with -fsanitize=address,undefined as a
stand-alone program over exact-size heap buffers (tools/content_hostcheck.cpp), equal the restatement bit for bit over the matrix of
sizes, alignments and block splits the GPU test runs."""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import content_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M = r"slideo_matcher\s*\*\s*m"
CALLS = {
    "slideo_matcher_content_begin": _M + r",\s*int32_t level",
    "slideo_matcher_content_end": _M,
    "slideo_matcher_content_info": _M + r",\s*int32_t\s*\*\s*aw,\s*int32_t\s*\*\s*ah,\s*int32_t\s*\*\s*frames,\s*int32_t\s*\*\s*level",
    "slideo_matcher_content_counts": _M + r",\s*uint32_t\s*\*\s*out,\s*int64_t capacity_elems,\s*int32_t\s*\*\s*aw,\s*int32_t\s*\*\s*ah,\s*int32_t\s*\*\s*frames",
    "slideo_matcher_content_box": _M + r",\s*int32_t min_share_ppm,\s*int32_t min_fill_ppm,\s*int32_t\s*\*\s*box\s*,\s*int64_t\s*\*\s*n_content,\s*uint32_t\s*\*\s*fill_out\s*,"
                                       r"\s*int64_t fill_capacity_elems",
}
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
ARGTYPES = {
    "slideo_matcher_content_begin": [vp, i32],
    "slideo_matcher_content_end": [vp],
    "slideo_matcher_content_info": [vp, vp, vp, vp, vp],
    "slideo_matcher_content_counts": [vp, vp, i64, vp, vp, vp],
    "slideo_matcher_content_box": [vp, i32, i32, vp, vp, vp, i64],
}


def test_header_declares_the_calls_with_their_signatures():
    src = open(os.path.join(ROOT, "include", "slideo_amd.h")).read()
    assert "Frame content box" in src
    assert "finding a quad other than the axis-aligned content box" in src and "finding the quad;" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, args in CALLS.items():
        assert re.search(r"\bint32_t\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), name
    assert "#define SLIDEO_ABI_VERSION 7" in src


def test_library_exports_them_at_abi_7_and_refuses_null_handles(capi):
    L = capi.lib()
    for name, argtypes in ARGTYPES.items():
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
        assert getattr(L, name).argtypes == argtypes, name
        # every call: SLIDEO_ERR_INVALID_ARG for a null handle, without a device
        zeros = [None if t is vp else t(0) for t in argtypes]
        assert getattr(L, name)(*zeros) == 1, name
    assert L.slideo_abi_version() == 7
    assert C.sizeof(capi.Config) == 168                          # entry points only: no new slideo_config field


def test_python_surface_and_rust_declarations(capi):
    for meth in ("content_begin", "content_end", "content_info", "content_counts", "content_box"):
        assert callable(getattr(capi.Matcher, meth)), meth
    from slideo_amd import matching as mt
    sig = inspect.signature(mt.learn_frame_region)
    assert list(sig.parameters) == ["matcher", "frame_batches", "level", "min_share", "min_fill", "inset", "out_size"]
    for k in ("level", "min_share", "min_fill"):                 # no default is chosen
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is inspect.Parameter.empty
    assert sig.parameters["inset"].default == 0 and sig.parameters["out_size"].default is None
    ffi = open(os.path.join(ROOT, "crates", "matching-hip", "src", "ffi.rs")).read()
    for name in CALLS:
        assert re.search(r"pub fn %s\(" % name, ffi), name


class _Fake:
    """A matcher that records the calls; the accumulator analyses the frames at `analysed` (None: at their own size)."""

    def __init__(self, box, analysed=None):
        self.log, self.box, self.analysed, self.size = [], box, analysed, (0, 0)

    def content_begin(self, level):
        self.log.append(("begin", level))

    def observe_frames(self, frames):
        self.log.append(("observe", len(frames)))
        self.size = (np.shape(frames)[2], np.shape(frames)[1])

    def content_info(self):
        aw, ah = self.analysed or self.size
        return {"aw": aw, "ah": ah, "frames": 3, "level": 32}

    def content_box(self, min_share, min_fill):
        self.log.append(("box", min_share, min_fill))
        return self.box, 7, None, None

    def content_end(self):
        self.log.append(("end",))


def test_learn_frame_region_runs_begin_observe_box_end():
    from slideo_amd import matching as mt
    a, b = np.zeros((2, 36, 64, 3), np.uint8), np.zeros((1, 36, 64, 3), np.uint8)
    f = _Fake((8, 0, 56, 36))
    got = mt.learn_frame_region(f, [a, b], level=32, min_share=0.5, min_fill=0.25)
    assert f.log == [("begin", 32), ("observe", 2), ("observe", 1), ("box", 0.5, 0.25), ("end",)]
    # the quad: the box's corner pixel centres; the output: the box's own size
    assert got == (64, 36, [(8.0, 0.0), (55.0, 0.0), (55.0, 35.0), (8.0, 35.0)], 48, 36)
    # inset shrinks every side; out_size replaces the box's size
    got = mt.learn_frame_region(_Fake((8, 0, 56, 36)), [a], level=1, min_share=0.1, min_fill=0.2, inset=3)
    assert got == (64, 36, [(11.0, 3.0), (52.0, 3.0), (52.0, 32.0), (11.0, 32.0)], 42, 30)
    got = mt.learn_frame_region(_Fake((8, 0, 56, 36)), [a], level=1, min_share=0.1, min_fill=0.2, inset=1, out_size=(480, 360))
    assert got == (64, 36, [(9.0, 1.0), (54.0, 1.0), (54.0, 34.0), (9.0, 34.0)], 480, 360)
    # an empty box, and one narrower than 2 pixels after the inset
    for box, inset in (((0, 0, 0, 0), 0), ((10, 4, 11, 30), 0), ((10, 4, 15, 30), 2), ((10, 4, 40, 9), 2)):
        g = _Fake(box)
        with pytest.raises(ValueError, match="empty or narrower than 2"):
            mt.learn_frame_region(g, [a], level=32, min_share=0.5, min_fill=0.25, inset=inset)
        assert g.log[-1] == ("end",)
    assert mt.learn_frame_region(_Fake((10, 4, 16, 30)), [a], level=32, min_share=0.5, min_fill=0.25, inset=2)[3:] == (2, 22)
    # analysed at another size than the frames': the box is not in source coordinates
    g = _Fake((8, 0, 24, 18), analysed=(32, 18))
    with pytest.raises(ValueError, match="not in source coordinates"):
        mt.learn_frame_region(g, [a], level=32, min_share=0.5, min_fill=0.25)
    assert g.log[-1] == ("end",)

    class Failing(_Fake):
        def observe_frames(self, frames):
            raise RuntimeError("boom")

    g = Failing((0, 0, 4, 4))
    with pytest.raises(RuntimeError):
        mt.learn_frame_region(g, [a], level=1, min_share=0.1, min_fill=0.1)
    assert g.log == [("begin", 1), ("end",)]                      # the accumulator is ended on the way out


# ---- the restatement on hand-computed cases ------------------------------------------------------------------------------------

def test_restatement_lit_by_hand():
    level = 40
    img = np.zeros((5, 6, 3), np.uint8)                          # 6 columns x 5 rows
    img[0, 0] = [level, level, level]                            # max == level: not lit
    img[0, 1] = [level + 1, 0, 0]                                # max == level + 1, in B, G and R in turn: lit
    img[1, 2] = [0, level + 1, 0]
    img[2, 3] = [0, 0, level + 1]
    img[3, 4] = [level, level - 1, 0]
    img[4, 5] = [255, 255, 255]
    want = np.zeros((5, 6), bool)
    want[0, 1] = want[1, 2] = want[2, 3] = want[4, 5] = True
    assert np.array_equal(R.lit(img, level), want)
    # level 0: whatever is not black; level 254: only a 255
    assert R.lit(img, 0).sum() == 6 and not R.lit(img, 0)[1, 1]
    assert np.array_equal(R.lit(img, 254), img.max(axis=2) == 255) and R.lit(img, 254).sum() == 1
    img[0, 0] = [254, 254, 254]
    assert not R.lit(img, 254)[0, 0]
    # counts and frames, in one observation and across calls
    f = np.stack([img, np.zeros_like(img), img])
    lit, frames = R.counts(f, level)
    assert frames == 3 and lit.dtype == np.uint32 and lit[4, 5] == 2 and lit[0, 0] == 2 and lit[1, 1] == 0
    acc = R.Accumulator(level).observe(f[:1]).observe(f[1:])
    assert acc.frames == 3 and np.array_equal(acc.lit, lit)


def test_restatement_share_and_fill_are_strict():
    lit = np.array([[1, 2, 0, 4]], np.uint32)
    # 2 * 1e6 == 500000 * 4: equality is not content; one ppm less is
    assert R.content(lit, 4, 500000).tolist() == [[False, False, False, True]]
    assert R.content(lit, 4, 499999).tolist() == [[False, True, False, True]]
    assert R.content(lit, 4, 1000000).tolist() == [[False, False, False, False]]    # no count exceeds frames
    assert R.content(lit, 4, 0).tolist() == [[True, True, False, True]]             # share 0: every pixel that was ever lit
    big = np.array([[2147483647]], np.uint32)                                       # the products need 64 bits
    assert R.content(big, 2147483647, 999999).tolist() == [[True]] and R.content(big, 2147483647, 1000000).tolist() == [[False]]
    # fills: 4 columns x 4 rows, rows with 0, 1, 2 and 4 content pixels
    lit = np.array([[0, 0, 0, 0], [0, 3, 0, 0], [0, 3, 3, 0], [3, 3, 3, 3]], np.uint32)
    rf, cf, n = R.fills(lit, 3, 500000)
    assert rf.tolist() == [0, 1, 2, 4] and cf.tolist() == [1, 3, 2, 1] and n == 7
    # min_fill 0.5: a row with exactly 2 of 4 is not a content row, a column with exactly 2 of 4 is not a content column
    assert R.box(lit, 3, 500000, 500000)[0] == (1, 3, 2, 4)
    assert R.box(lit, 3, 500000, 499999)[0] == (1, 2, 3, 4)
    assert R.box(lit, 3, 500000, 0)[0] == (0, 1, 4, 4)                              # fill 0: every row and column that has any
    assert R.box(lit, 3, 500000, 1000000)[0] == (0, 0, 0, 0)                        # a full row is still not above 1.0
    assert R.box(lit, 3, 500000, 750000)[0] == (0, 0, 0, 0)                         # a content row (3) but no content column: empty


def test_restatement_boxes_by_hand():
    frames = 2
    dark = np.zeros((6, 8), np.uint32)
    b, n, rf, cf = R.box(dark, frames, 0, 0)
    assert b == (0, 0, 0, 0) and n == 0 and not rf.any() and not cf.any()          # empty
    full = np.full((6, 8), 2, np.uint32)
    b, n, rf, cf = R.box(full, frames, 500000, 250000)
    assert b == (0, 0, 8, 6) and n == 48 and (rf == 8).all() and (cf == 6).all()    # touching all four borders
    # a pillarbox: columns 2..5 lit in both frames; a single lit speck in the left bar
    pb = np.zeros((6, 8), np.uint32)
    pb[:, 2:6] = 2
    assert R.box(pb, frames, 500000, 250000)[0] == (2, 0, 6, 6)
    pb[3, 0] = 2
    b, n, rf, cf = R.box(pb, frames, 500000, 250000)
    # the speck's column holds 1 of 6 pixels: 1e6 > 250000 * 6 is false — min_fill above one pixel per column keeps the box
    assert b == (2, 0, 6, 6) and n == 25 and cf[0] == 1 and rf[3] == 5
    assert R.box(pb, frames, 500000, 100000)[0] == (0, 0, 6, 6)                     # below one pixel per column it widens
    # a letterbox the same way, the speck in the top bar
    lb = np.zeros((6, 8), np.uint32)
    lb[1:5] = 2
    lb[0, 7] = 2
    assert R.box(lb, frames, 500000, 250000)[0] == (0, 1, 8, 5)                     # 1 of 8: 1e6 > 250000 * 8 is false


# ---- the kernels' per-thread bodies, compiled for the host -----------------------------------------------------------------------

def _build(tmp, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror"] + extra +
                          ["-I", os.path.join(ROOT, "slideo_amd", "csrc"), os.path.join(ROOT, "tools", "content_hostcheck.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def hostchecks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("content")
    return {"plain": _build(tmp, "hostcheck", []),
            "sanitized": _build(tmp, "hostcheck_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def _run(hostchecks, tmp_path, frames, kind, ofs, level, ppm, split=()):
    """-> per build {lit, row_fill, col_fill, n_content, said}"""
    n, h, w, _ = frames.shape
    stride = R.strides(w)[kind]
    buf = R.padded(frames, stride, 0, fill=0xFF)                   # (padding of 255: lit, were it ever read as a pixel)
    cin, cout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    split = tuple(split) + (0,) * (4 - len(split))
    with open(cin, "wb") as f:
        f.write(struct.pack("<11i", w, h, stride, n, ofs, level, ppm, *split) + buf.tobytes())
    out = {}
    for name, exe in hostchecks.items():
        if os.path.exists(cout):
            os.remove(cout)
        said = subprocess.check_output([exe, cin, cout]).decode()
        raw = open(cout, "rb").read()
        px = w * h
        assert len(raw) == 4 * (px + h + w) + 8
        out[name] = dict(lit=np.frombuffer(raw, np.uint32, px).reshape(h, w), row_fill=np.frombuffer(raw, np.uint32, h, px * 4),
                         col_fill=np.frombuffer(raw, np.uint32, w, (px + h) * 4), n_content=int(np.frombuffer(raw, np.int64, 1, (px + h + w) * 4)[0]),
                         said=said)
    return out


def _held(got, frames, level, ppm, what):
    lit, n = R.counts(frames, level)
    rf, cf, nc = R.fills(lit, n, ppm)
    for name, g in got.items():
        assert np.array_equal(g["lit"], lit), (what, name, int((g["lit"] != lit).sum()))
        assert np.array_equal(g["row_fill"], rf) and np.array_equal(g["col_fill"], cf) and g["n_content"] == nc, (what, name)


@pytest.mark.parametrize("w,h", R.COUNT_SIZES + [R.BIG[:2]], ids=lambda v: str(v))
def test_host_build_of_content_kernel_equals_the_restatement(hostchecks, tmp_path, w, h):
    for n in ((R.BIG[2],) if (w, h) == R.BIG[:2] else R.FRAME_COUNTS):
        frames = R.level_frames(n, h, w, w * 7 + h + n)
        assert w * h < 4 or 0 < int(R.counts(frames, R.LEVEL)[0].astype(bool).sum()) < w * h
        for kind, ofs in R.layouts(n):
            got = _run(hostchecks, tmp_path, frames, kind, ofs, R.LEVEL, 500000)
            _held(got, frames, R.LEVEL, 500000, (n, kind, ofs))
            dwords = ofs == 0 and R.strides(w)[kind] % 4 == 0 and (h * R.strides(w)[kind]) % 4 == 0
            for g in got.values():
                assert ("in4 1" in g["said"]) == dwords, (n, kind, ofs, g["said"])       # the dword path ran exactly where it may
                assert ("own4 1" in g["said"]) == (w % 4 == 0), g["said"]
        if n == sum(R.SPLIT):                                      # the same frames over three launches
            for kind in ("tight", "odd"):
                got = _run(hostchecks, tmp_path, frames, kind, 0, R.LEVEL, 500000, R.SPLIT)
                _held(got, frames, R.LEVEL, 500000, ("split", kind))
                assert all("launches 3" in g["said"] for g in got.values())
    # level 0 and 254 through the kernel body
    frames = R.level_frames(3, h, w, w + h)
    frames[0, 0, 0] = [255, 0, 1]
    for level in (0, 254):
        _held(_run(hostchecks, tmp_path, frames, "tight", 0, level, 0), frames, level, 0, ("level", level))


@pytest.mark.parametrize("w,h", R.READ_SIZES, ids=lambda v: str(v))
def test_host_build_of_content_fill_kernel_equals_the_restatement(hostchecks, tmp_path, w, h):
    frames = R.read_frames(w, h)
    lit, n = R.counts(frames, R.LEVEL)
    assert n == R.READ_FRAMES and (lit[h // 2] == 2).all()       # the equality of share 0.5 is in the content
    seen = set()
    for share in R.SHARES:
        ppm = int(round(share * 1000000))
        _held(_run(hostchecks, tmp_path, frames, "tight", 0, R.LEVEL, ppm), frames, R.LEVEL, ppm, ("share", share))
        seen.add(R.fills(lit, n, ppm)[2])
    assert 0 in seen and (w * h == 1 or len(seen) == 3)           # share 1.0: nothing is content
