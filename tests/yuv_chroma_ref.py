"""Test-side numpy restatement of include/slideo_amd.h "YUV chroma filter": the weight tables of a (filter, sampling) pair and the
BGR8 image a 4:2:0, 4:2:2 or packed 4:2:2 frame stands for under a description and a chroma filter.  Written from the header, not
from csrc/: the layouts, the 8-bit value of a sample and the coefficients come from tests/yuv_desc_ref.py and
tests/yuv_sampling_ref.py, the filter is restated here in the header's own general form (three taps per axis, every index clamped).
Also the conversion cases the CPU host check and the GPU tap test share.  `layout`: anything with the fields of
slideo_yuv420_layout; strides and offsets are BYTES whatever the container."""
import numpy as np

import yuv_desc_ref as D
import yuv_sampling_ref as S

NEAREST, LEFT, CENTER, TOPLEFT = 0, 1, 2, 3
FILTERS = (LEFT, CENTER, TOPLEFT)
FILTER_NAMES = {NEAREST: "nearest", LEFT: "left", CENTER: "center", TOPLEFT: "topleft"}
S420, S422, S444, S422P = S.S420, S.S422, S.S444, S.S422P
NONE = ((0, 4, 0), (0, 4, 0))
COSITED = ((0, 4, 0), (0, 2, 2))
CENTRED = ((1, 3, 0), (0, 3, 1))
FORMATS = {S420: D.FORMATS, S422: S.FORMATS[S422], S422P: S.FORMATS[S422P], S444: S.FORMATS[S444]}
DEPTHS = {S420: D.DEPTHS, S422: D.DEPTHS, S422P: (D.D8,), S444: D.DEPTHS}
SAMPLINGS = (S420, S422, S422P)                 # the samplings a filter changes


def weights(filt, sampling):
    """(wh, wv): [parity][sample k-1, k, k+1] in quarters; an axis that is not interpolated is (0, 4, 0) twice."""
    if filt == NEAREST or sampling == S444:
        return NONE, NONE
    wh = CENTRED if filt == CENTER else COSITED
    if sampling != S420:
        return wh, NONE
    return wh, (COSITED if filt == TOPLEFT else CENTRED)


def weights12(filt, sampling):
    wh, wv = weights(filt, sampling)
    return [x for t in (wh, wv) for row in t for x in row]


def sampling_of(fmt):
    return S420 if fmt in D.FORMATS else S.sampling_of(fmt)


def _taps(C, w3, axis):
    """sum_i w3[parity][i] * C[k - 1 + i] along `axis` for the 2 * n positions x (k = x >> 1, parity = x & 1), indices clamped."""
    n = C.shape[axis]
    x = np.arange(2 * n)
    k, par = x >> 1, x & 1
    wt = np.asarray(w3, np.int64)
    out = 0
    for i in range(3):
        idx = np.clip(k - 1 + i, 0, n - 1)
        wi = wt[par, i]
        shape = [1, 1]
        shape[axis] = -1
        out = out + np.take(C, idx, axis) * wi.reshape(shape)
    return out


def chroma_at_pixels(C, filt, sampling):
    """U8 (or V8) of every pixel from one chroma plane's s8 values C [chh, cw]."""
    wh, wv = weights(filt, sampling)
    if sampling == S444:
        return C
    H = _taps(np.asarray(C, np.int64), wh, 1)
    if sampling == S420:
        return (_taps(H, wv, 0) + 8) >> 4
    return (H + 2) >> 2


def sample_offsets(w, h, layout, depth, sampling):
    return D.plane_offsets(w, h, layout, depth) if sampling == S420 else S.sample_offsets(w, h, layout, depth, sampling)


def to_bgr(buf, w, h, layout, desc, sampling, filt):
    """The BGR8 image [h, w, 3] one frame stands for under desc = (matrix, range, depth), `sampling` and the chroma filter."""
    matrix, rng, depth = desc
    CY, CUB, CUG, CVG, CVR, yofs, shift = D.coefficients(matrix, rng)
    half = 1 << (shift - 1)
    oy, ou, ov = sample_offsets(w, h, layout, depth, sampling)
    Y, U, V = (D.s8(D.samples(buf, o, depth), depth) for o in (oy, ou, ov))
    U, V = chroma_at_pixels(U, filt, sampling), chroma_at_pixels(V, filt, sampling)
    u, v = U - 128, V - 128
    y = np.maximum(Y - yofs, 0) * CY
    r = (y + half + CVR * v) >> shift
    g = (y + half + CVG * v + CUG * u) >> shift
    b = (y + half + CUB * u) >> shift
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def frames_to_yuv(frames, layout, frame_bytes, desc, sampling):
    if sampling == S420:
        return D.frames_to_yuv(frames, layout, frame_bytes, desc)
    return S.frames_to_yuv(frames, layout, frame_bytes, desc, sampling)


def frames_to_bgr(yuv, w, h, layout, desc, sampling, filt):
    return np.stack([to_bgr(f, w, h, layout, desc, sampling, filt) for f in yuv])


# ---- the conversion cases the CPU host check and the GPU tap test share -------------------------------------------------------------
# The kernel's thread is 4 pixels wide, a wave 64 threads (256 pixels), a block 4 thread rows; under 4:2:0 a thread row is 2 luma
# rows.  2x2: every tap clamped; 4x2, 2x4; 6x6: a ragged thread; 254 / 256 / 258: one short of, at, and one past a wave's span (the
# halo loads of the first and the last lane); 510 / 514: the same for two; 66x34: more than one block of rows.
SIZES = [(2, 2), (4, 2), (2, 4), (6, 6), (8, 8), (10, 6), (254, 6), (256, 8), (258, 10), (510, 18), (514, 16), (66, 34)]
SIZES_422_ODD = [(2, 1), (6, 3), (258, 5)]


def sizes(sampling):
    return SIZES + (SIZES_422_ODD if sampling != S420 else [])


def layouts(capi, fmt, w, h, depth):
    """[(name, layout, frame bytes)]: tight, pitched (every wide load applies) and skewed (they miss), by the sampling's own rules.
    Under 4:2:0 the skewed pitch of 16-bit containers is 4 mod 8, where interleaved chroma still takes its two-dword form: skewed2, a
    pitch = 2 mod 4, misses that too (interleaved only: a planar format's chroma rows would be odd)."""
    if sampling_of(fmt) != S420:
        return S.layouts(capi, fmt, w, h, depth)
    b = D.bps(depth)
    out = D.layouts(capi, fmt, w, h, depth)
    if b == 2 and fmt in ("nv12", "nv21"):
        p = -(-w * b // 64) * 64
        out.append(("skewed2",) + capi.yuv420_layout(fmt, w, h, pitch=p + 2, row_align=2, bytes_per_sample=b))
    return out


def random_frame(w, h, layout, frame_bytes, depth, sampling, seed):
    if sampling == S420:
        return D.random_frame(w, h, layout, frame_bytes, depth, seed)
    return S.random_frame(w, h, layout, frame_bytes, depth, sampling, seed)


def tap_cases(capi):
    """Every (sampling, depth, fmt, layout name, layout, frame bytes, w, h) of the matrix; the filter and the colour pair rotate
    over them in the caller."""
    for sampling in SAMPLINGS:
        for depth in DEPTHS[sampling]:
            for fmt in FORMATS[sampling]:
                for (w, h) in sizes(sampling):
                    for name, L, fb in layouts(capi, fmt, w, h, depth):
                        yield sampling, depth, fmt, name, L, fb, w, h
