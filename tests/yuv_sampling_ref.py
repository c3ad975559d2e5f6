"""Test-side numpy restatement of include/slideo_amd.h "YUV sampling": the BGR8 image a 4:2:2, 4:4:4 or packed 4:2:2 frame stands
for under a description, written from the header, not from csrc/ (the coefficients and the 8-bit value of a sample come from
tests/yuv_desc_ref.py, the per-pixel formula is restated here).  Also the forward direction (BGR -> a frame of each sampling), the
tight layouts of slideo_yuv_layout_packed, a layout generator that hits and misses every wide load of the kernel, and random frames.
`layout`: anything with the fields of slideo_yuv420_layout; strides and offsets are BYTES whatever the container."""
import os
import re

import numpy as np

import yuv_desc_ref as D

S420, S422, S444, S422P = 0, 1, 2, 3
SAMPLING_NAMES = {S420: "420", S422: "422", S444: "444", S422P: "422_packed"}
FORMAT_VALUES = {"i422": 16, "yv16": 17, "nv16": 18, "nv61": 19, "yuy2": 20, "uyvy": 21, "yvyu": 22, "vyuy": 23,
                 "i444": 24, "yv24": 25, "nv24": 26, "nv42": 27}
FORMATS = {S422: ("i422", "yv16", "nv16", "nv61"), S444: ("i444", "yv24", "nv24", "nv42"), S422P: ("yuy2", "uyvy", "yvyu", "vyuy")}
DEPTHS = {S422: D.DEPTHS, S444: D.DEPTHS, S422P: (D.D8,)}
PACKED_OFFSETS = {"yuy2": (1, 3), "yvyu": (3, 1), "uyvy": (0, 2), "vyuy": (2, 0)}
# per format: (U first?, interleaved?)
_KIND = {"i422": (True, False), "yv16": (False, False), "nv16": (True, True), "nv61": (False, True),
         "i444": (True, False), "yv24": (False, False), "nv24": (True, True), "nv42": (False, True)}
SAMPLINGS = (S422, S444, S422P)


def sampling_of(fmt):
    return next(s for s, names in FORMATS.items() if fmt in names)


def yuv_tx():
    """The kernel's block width in threads (4 columns each), read from its source: the tap test derives one width from it."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slideo_amd", "csrc", "yuv420.hip.h")).read()
    return int(re.search(r"YUV_TX = (\d+)", src).group(1))


def sizes(sampling):
    """(w, h) of the conversion cases: one ragged thread; a tail of 2; (4:4:4) tails of 3 and 1; an odd height; whole blocks; a
    width beyond one block's columns."""
    s = [(2, 1), (6, 3)]
    if sampling == S444:
        s += [(7, 5), (9, 2)]
    return s + [(34, 5), (64, 36), (4 * yuv_tx() * 2 + 6, 3)]


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def make_layout(capi, fmt, w, h, b=1, pitch=None, rows=None):
    """(layout, frame bytes) of `fmt` by the header's words.  pitch: bytes per luma row (packed: per row of the one plane); planar
    4:2:2 chroma rows take pitch / 2, interleaved 4:4:4 chroma rows 2 * pitch, the others pitch.  rows: rows every plane is allotted
    (>= h).  Neither: the tight layout."""
    s = sampling_of(fmt)
    ah = rows or h
    L = capi.Yuv420Layout()
    if s == S422P:
        p = pitch or 2 * w
        L.y_stride, L.uv_stride, L.uv_step = p, p, 4
        L.u_offset, L.v_offset = PACKED_OFFSETS[fmt]
        return L, p * ah
    u_first, inter = _KIND[fmt]
    p = pitch or w * b
    luma = p * ah
    L.y_stride = p
    if inter:
        cp = p if s == S422 else 2 * p
        L.uv_stride, L.uv_step = cp, 2
        L.u_offset, L.v_offset = (luma, luma + b) if u_first else (luma + b, luma)
        return L, luma + cp * ah
    cp = p // 2 if s == S422 else p
    L.uv_stride, L.uv_step = cp, 1
    L.u_offset, L.v_offset = (luma, luma + cp * ah) if u_first else (luma + cp * ah, luma)
    return L, luma + 2 * cp * ah


def _align(x, a):
    return -(-x // a) * a


def layouts(capi, fmt, w, h, depth):
    """[(name, layout, frame bytes)].  tight.  pitched: 64-byte pitch, 16 aligned rows — every wide load applies.  skewed: a pitch
    that misses the wide loads — 8-bit: pitch = 2 mod 4 (luma's and interleaved chroma's dword, packed's 8 and 4 bytes; planar
    4:2:2 chroma rows are odd: the 2-byte load); 16-bit: pitch = 4 mod 8 (luma's and interleaved 4:2:2 chroma's 8 bytes; planar
    4:2:2 chroma rows are 2 mod 4: the dword), and for interleaved 4:4:4, whose chroma rows are always dword-aligned, pitch = 2 mod 4
    with an odd number of rows: the chroma plane starts 2 mod 4.  skewed4: pitch = 4 mod 8 with 2 aligned rows: the two-dword forms of
    the packed load and of 8-bit interleaved 4:4:4 chroma."""
    b = D.bps(depth)
    s = sampling_of(fmt)
    p = _align((2 * w) if s == S422P else w * b, 64)
    out = [("tight",) + make_layout(capi, fmt, w, h, b), ("pitched",) + make_layout(capi, fmt, w, h, b, p, _align(h, 16))]
    if b == 2 and s == S444 and _KIND[fmt][1]:
        out.append(("skewed",) + make_layout(capi, fmt, w, h, b, p + 2, h | 1))
    else:
        out.append(("skewed",) + make_layout(capi, fmt, w, h, b, p + 2 * b, h))
    out.append(("skewed4",) + make_layout(capi, fmt, w, h, b, p + 4, _align(h, 2)))
    return out


# ---- where the samples lie ----------------------------------------------------------------------------------------------------------
def sample_offsets(w, h, layout, depth, sampling):
    """Byte offsets of the samples, at SAMPLE resolution: Y [h, w]; U, V [h, w/2] (both 4:2:2 forms) or [h, w] (4:4:4)."""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    if sampling == S422P:
        xm = np.arange(w // 2)[None, :]
        oy = y * layout.y_stride + 2 * x + ((layout.u_offset & 1) ^ 1)
        return oy, y * layout.y_stride + layout.u_offset + 4 * xm, y * layout.y_stride + layout.v_offset + 4 * xm
    b = D.bps(depth)
    cx = np.arange(w // 2 if sampling == S422 else w)[None, :]
    crow = y * layout.uv_stride + cx * layout.uv_step * b
    return y * layout.y_stride + x * b, layout.u_offset + crow, layout.v_offset + crow


def to_bgr(buf, w, h, layout, desc, sampling):
    """The BGR8 image [h, w, 3] one frame stands for under desc = (matrix, range, depth) and `sampling`: "YUV colour
    description"'s formula, pixel (x, y) taking chroma (x/2, y) (4:2:2) or (x, y) (4:4:4)."""
    matrix, rng, depth = desc
    CY, CUB, CUG, CVG, CVR, yofs, shift = D.coefficients(matrix, rng)
    half = 1 << (shift - 1)
    oy, ou, ov = sample_offsets(w, h, layout, depth, sampling)
    Y, U, V = (D.s8(D.samples(buf, o, depth), depth) for o in (oy, ou, ov))
    if sampling != S444:
        U, V = np.repeat(U, 2, 1), np.repeat(V, 2, 1)
    u, v = U - 128, V - 128
    y = np.maximum(Y - yofs, 0) * CY
    r = (y + half + CVR * v) >> shift
    g = (y + half + CVG * v + CUG * u) >> shift
    b = (y + half + CUB * u) >> shift
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


# ---- the forward direction (an encoder's side: its exact rounding is not part of any contract) -------------------------------------
def from_bgr(bgr, matrix, rng, sampling):
    """A BGR8 image [h, w, 3] in float64 -> 8-bit-scaled (Y, U, V) as floats; 4:2:2: chroma the mean of each pixel pair."""
    f = np.asarray(bgr, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    Kr, Kb = D.K[matrix]
    y = Kr * r + (1.0 - Kr - Kb) * g + Kb * b
    cb, cr = (b - y) / (2.0 * (1.0 - Kb)), (r - y) / (2.0 * (1.0 - Kr))
    if rng == D.FULL:
        Y, U, V = y, 128.0 + cb, 128.0 + cr
    else:
        Y, U, V = 16.0 + y * 219.0 / 255.0, 128.0 + cb * 224.0 / 255.0, 128.0 + cr * 224.0 / 255.0
    if sampling != S444:
        U, V = (c.reshape(c.shape[0], c.shape[1] // 2, 2).mean(axis=2) for c in (U, V))
    return Y, U, V


def pack(Y, U, V, w, h, layout, frame_bytes, depth, sampling, seed=0):
    """One frame's bytes from RAW container values (int arrays at sample resolution); the bytes no sample covers are random."""
    rng = np.random.default_rng(h * 7919 + w + seed)
    buf = rng.integers(0, 256, frame_bytes, dtype=np.uint8)
    for off, p in zip(sample_offsets(w, h, layout, depth, sampling), (Y, U, V)):
        p = np.asarray(p, np.int64)
        buf[off] = (p & 255).astype(np.uint8)
        if depth != D.D8:
            buf[off + 1] = (p >> 8).astype(np.uint8)
    return buf


def frames_to_yuv(frames, layout, frame_bytes, desc, sampling):
    """[n, h, w, 3] BGR frames -> [n, frame_bytes] frames of `sampling` under desc in `layout`."""
    matrix, rng, depth = desc
    out = []
    for f in frames:
        h, w = f.shape[:2]
        Y, U, V = from_bgr(f, matrix, rng, sampling)
        out.append(pack(D.quantise(Y, depth), D.quantise(U, depth), D.quantise(V, depth), w, h, layout, frame_bytes, depth, sampling))
    return np.stack(out)


def random_frame(w, h, layout, frame_bytes, depth, sampling, seed):
    """Raw values uniform over the sample range with the range's corner values sprinkled in (yuv_desc_ref.random_raw's planes, at
    this sampling's chroma size)."""
    rng = np.random.default_rng(seed)
    cw = w if sampling == S444 else w // 2

    def plane(ph, pw):
        return D.random_raw(2 * pw, 2 * ph, depth, rng)[1]            # (its chroma plane is [ph, pw])
    return pack(plane(h, w), plane(h, cw), plane(h, cw), w, h, layout, frame_bytes, depth, sampling, seed)
