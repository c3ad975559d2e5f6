"""Test-side numpy restatement of the YUV 4:2:0 -> BGR8 conversion of include/slideo_amd.h ("YUV 4:2:0 frames"): OpenCV 4.x
cvtColor(COLOR_YUV2BGR_NV12 / _NV21 / _I420 / _YV12), BT.601 limited range, nearest chroma, fixed point with SHIFT 20 (recalled).
Also the forward direction the tests use to turn synthetic BGR frames into decoder-shaped 4:2:0 frames, and a packer for
pitched layouts.  `layout`: anything with the fields of slideo_yuv420_layout (the ctypes Yuv420Layout)."""
import numpy as np

CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527
SHIFT, HALF = 20, 1 << 19


def planes(buf, w, h, layout):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) of one frame's bytes."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    ch, cw = h // 2, w // 2
    rows = np.arange(h)[:, None] * layout.y_stride + np.arange(w)[None, :]
    crow = np.arange(ch)[:, None] * layout.uv_stride + np.arange(cw)[None, :] * layout.uv_step
    return buf[rows], buf[layout.u_offset + crow], buf[layout.v_offset + crow]


def to_bgr(buf, w, h, layout):
    """The BGR8 image [h, w, 3] of one 4:2:0 frame, bit for bit as the library makes it."""
    Y, U, V = planes(buf, w, h, layout)
    u = np.repeat(np.repeat(U.astype(np.int64) - 128, 2, 0), 2, 1)
    v = np.repeat(np.repeat(V.astype(np.int64) - 128, 2, 0), 2, 1)
    y = np.maximum(Y.astype(np.int64) - 16, 0) * CY
    r = (y + HALF + CVR * v) >> SHIFT
    g = (y + HALF + CVG * v + CUG * u) >> SHIFT
    b = (y + HALF + CUB * u) >> SHIFT
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def float_bgr(Y, U, V):
    """The BT.601 limited-range formula in floating point (the textbook form; agrees with to_bgr within +-1)."""
    y = 1.164 * np.maximum(np.asarray(Y, np.float64) - 16, 0)
    u, v = np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    r, g, b = y + 1.596 * v, y - 0.813 * v - 0.391 * u, y + 2.018 * u
    return np.clip(np.rint(np.stack([b, g, r], -1)), 0, 255)


def from_bgr(bgr):
    """Forward BT.601 limited range of a BGR8 image [h, w, 3] (even sides): (Y, U, V), chroma the 2x2 mean."""
    f = np.asarray(bgr, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    Y = 16 + 0.257 * r + 0.504 * g + 0.098 * b
    U = 128 - 0.148 * r - 0.291 * g + 0.439 * b
    V = 128 + 0.439 * r - 0.368 * g - 0.071 * b
    sub = lambda c: c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return q(Y), q(sub(U)), q(sub(V))


def pack(Y, U, V, layout, frame_bytes, fill=None):
    """One frame's bytes in `layout` (frame_bytes long; the bytes no plane covers are `fill`, random when None)."""
    h, w = Y.shape
    rng = np.random.default_rng(h * 7919 + w)
    buf = rng.integers(0, 256, frame_bytes, dtype=np.uint8) if fill is None else np.full(frame_bytes, fill, np.uint8)
    ch, cw = h // 2, w // 2
    buf[np.arange(h)[:, None] * layout.y_stride + np.arange(w)[None, :]] = Y
    crow = np.arange(ch)[:, None] * layout.uv_stride + np.arange(cw)[None, :] * layout.uv_step
    buf[layout.u_offset + crow] = U
    buf[layout.v_offset + crow] = V
    return buf


def frames_to_yuv(frames, layout, frame_bytes):
    """[n, h, w, 3] BGR frames -> [n, frame_bytes] 4:2:0 frames in `layout`."""
    return np.stack([pack(*from_bgr(f), layout, frame_bytes) for f in frames])
