"""Test-side numpy restatement of include/slideo_amd.h "YUV colour description": the coefficients of a (matrix, range) pair by the
header's float64 rule, the 8-bit value of a sample under each depth, and the BGR8 image a 4:2:0 frame stands for under a
description.  Written from the header, not from csrc/.  Also the forward direction (BGR -> 4:2:0 under a description) and packers
the tests use to make decoder-shaped frames.  `layout`: anything with the fields of slideo_yuv420_layout; strides and offsets are
BYTES whatever the container."""
import numpy as np

BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
D8, D10_MSB, D10_LSB = 0, 1, 2
SHIFT, HALF = 20, 1 << 19
K = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}
OPENCV_601_LIMITED = (1220542, 2116026, -409993, -852492, 1673527, 16, 20)
PAIRS = [(m, r) for m in (BT601, BT709) for r in (LIMITED, FULL)]
DEPTHS = (D8, D10_MSB, D10_LSB)


def bps(depth):
    return 1 if depth == D8 else 2


def rule(matrix, rng):
    """(CY, CUB, CUG, CVG, CVR, y_offset, SHIFT) by the header's rule, in float64."""
    Kr, Kb = np.float64(K[matrix][0]), np.float64(K[matrix][1])
    Kg = np.float64(1.0) - Kr - Kb
    sy = np.float64(1.0) if rng == FULL else np.float64(255.0) / np.float64(219.0)
    sc = np.float64(1.0) if rng == FULL else np.float64(255.0) / np.float64(224.0)
    one = np.float64(1 << 20)
    two = np.float64(2.0)
    return (int(np.rint(sy * one)), int(np.rint(sc * two * (1.0 - Kb) * one)), -int(np.rint(sc * two * (1.0 - Kb) * Kb / Kg * one)),
            -int(np.rint(sc * two * (1.0 - Kr) * Kr / Kg * one)), int(np.rint(sc * two * (1.0 - Kr) * one)), 0 if rng == FULL else 16, SHIFT)


def coefficients(matrix, rng):
    return OPENCV_601_LIMITED if (matrix, rng) == (BT601, LIMITED) else rule(matrix, rng)


def samples(buf, offsets, depth):
    """The raw samples at byte `offsets` (any shape) of one frame's bytes: uint8, or little-endian uint16."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    if depth == D8:
        return buf[offsets].astype(np.int64)
    return buf[offsets].astype(np.int64) | (buf[offsets + 1].astype(np.int64) << 8)


def s8(raw, depth):
    if depth == D8:
        return raw
    if depth == D10_MSB:
        return raw >> 8
    return np.minimum(raw, 1023) >> 2


def plane_offsets(w, h, layout, depth):
    b = bps(depth)
    ch, cw = h // 2, w // 2
    rows = np.arange(h)[:, None] * layout.y_stride + np.arange(w)[None, :] * b
    crow = np.arange(ch)[:, None] * layout.uv_stride + np.arange(cw)[None, :] * layout.uv_step * b
    return rows, layout.u_offset + crow, layout.v_offset + crow


def to_bgr(buf, w, h, layout, desc):
    """The BGR8 image [h, w, 3] one 4:2:0 frame stands for under desc = (matrix, range, depth)."""
    matrix, rng, depth = desc
    CY, CUB, CUG, CVG, CVR, yofs, _ = coefficients(matrix, rng)
    oy, ou, ov = plane_offsets(w, h, layout, depth)
    Y, U, V = (s8(samples(buf, o, depth), depth) for o in (oy, ou, ov))
    u = np.repeat(np.repeat(U - 128, 2, 0), 2, 1)
    v = np.repeat(np.repeat(V - 128, 2, 0), 2, 1)
    y = np.maximum(Y - yofs, 0) * CY
    r = (y + HALF + CVR * v) >> SHIFT
    g = (y + HALF + CVG * v + CUG * u) >> SHIFT
    b = (y + HALF + CUB * u) >> SHIFT
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def from_bgr(bgr, matrix, rng):
    """Forward transform of a BGR8 image [h, w, 3] (even sides) in float64: 8-bit (Y, U, V) values as FLOATS (unrounded), chroma
    the 2x2 mean.  An encoder's side: its exact rounding is not part of any contract."""
    f = np.asarray(bgr, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    Kr, Kb = K[matrix]
    Kg = 1.0 - Kr - Kb
    y = Kr * r + Kg * g + Kb * b
    cb = (b - y) / (2.0 * (1.0 - Kb))
    cr = (r - y) / (2.0 * (1.0 - Kr))
    if rng == FULL:
        Y, U, V = y, 128.0 + cb, 128.0 + cr
    else:
        Y, U, V = 16.0 + y * 219.0 / 255.0, 128.0 + cb * 224.0 / 255.0, 128.0 + cr * 224.0 / 255.0
    sub = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
    return Y, sub(U), sub(V)


def quantise(plane, depth):
    """8-bit-scaled float values -> raw container values of `depth` (10-bit: value * 4, rounded, 0..1023; MSB: << 6)."""
    if depth == D8:
        return np.clip(np.rint(plane), 0, 255).astype(np.int64)
    v10 = np.clip(np.rint(np.asarray(plane) * 4.0), 0, 1023).astype(np.int64)
    return v10 << 6 if depth == D10_MSB else v10


def pack(Y, U, V, w, h, layout, frame_bytes, depth, seed=0):
    """One frame's bytes in `layout` from RAW container values (int arrays); the bytes no plane covers are random."""
    rng = np.random.default_rng(h * 7919 + w + seed)
    buf = rng.integers(0, 256, frame_bytes, dtype=np.uint8)
    for off, p in zip(plane_offsets(w, h, layout, depth), (Y, U, V)):
        p = np.asarray(p, np.int64)
        buf[off] = (p & 255).astype(np.uint8)
        if depth != D8:
            buf[off + 1] = (p >> 8).astype(np.uint8)
    return buf


def frames_to_yuv(frames, layout, frame_bytes, desc):
    """[n, h, w, 3] BGR frames -> [n, frame_bytes] 4:2:0 frames under desc in `layout`."""
    matrix, rng, depth = desc
    out = []
    for f in frames:
        h, w = f.shape[:2]
        Y, U, V = from_bgr(f, matrix, rng)
        out.append(pack(quantise(Y, depth), quantise(U, depth), quantise(V, depth), w, h, layout, frame_bytes, depth))
    return np.stack(out)


# ---- the conversion cases the CPU host check and the GPU tap test share ----------------------------------------------------------
SIZES = [(2, 2), (6, 4), (18, 10), (64, 36), (66, 34), (130, 70)]
FORMATS = ("nv12", "nv21", "i420", "yv12")
SPECIALS = {D8: (0, 16, 235, 240, 255), D10_MSB: (0, 64, 940, 960, 1023), D10_LSB: (0, 64, 940, 960, 1023)}


def _align(x, a):
    return -(-x // a) * a


def layouts(capi, fmt, w, h, depth):
    """[(name, layout, frame bytes)]: tight; pitched to 64 bytes with 16 aligned rows (every wide load applies); pitched so that the
    luma rows, and the planar chroma rows, miss the wide loads' alignment (8-bit: pitch = 2 mod 4; 16-bit: pitch = 4 mod 8, whose
    planar chroma rows are 2 mod 4)."""
    b = bps(depth)
    out = [("tight",) + capi.yuv420_layout(fmt, w, h, bytes_per_sample=b)]
    p = _align(w * b, 64)
    out.append(("pitched",) + capi.yuv420_layout(fmt, w, h, pitch=p, row_align=16, bytes_per_sample=b))
    out.append(("skewed",) + capi.yuv420_layout(fmt, w, h, pitch=p + 2 * b, row_align=2, bytes_per_sample=b))
    return out


def random_raw(w, h, depth, rng):
    """Raw container values (Y [h, w], U, V [h/2, w/2]): uniform over the sample range with the range's corner values sprinkled in;
    10_MSB: random low 6 bits under the value; 10_LSB: a share of values above 1023 (up to 65535)."""
    def plane(ph, pw):
        top = 256 if depth == D8 else 1024
        v = rng.integers(0, top, (ph, pw), dtype=np.int64)
        sp = np.asarray(SPECIALS[depth], np.int64)
        pick = rng.random((ph, pw)) < 0.25
        v[pick] = sp[rng.integers(0, len(sp), int(pick.sum()))]
        if depth == D10_MSB:
            v = (v << 6) | rng.integers(0, 64, (ph, pw), dtype=np.int64)
        if depth == D10_LSB:
            over = rng.random((ph, pw)) < 0.1
            v[over] = rng.integers(1024, 65536, int(over.sum()), dtype=np.int64)
        return v
    return plane(h, w), plane(h // 2, w // 2), plane(h // 2, w // 2)


def random_frame(w, h, layout, frame_bytes, depth, seed):
    rng = np.random.default_rng(seed)
    Y, U, V = random_raw(w, h, depth, rng)
    return pack(Y, U, V, w, h, layout, frame_bytes, depth, seed)
