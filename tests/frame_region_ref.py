"""The frame region's rectified image (include/slideo_amd.h "Frame region") restated in numpy: int64 and float64, no fused
operation, a whole image at once.  `rectify` is the definition the HIP kernels (csrc/frame_region.hip.h) are held to bit for bit;
`exact_coords` and `bilinear_f64` are the float64 ideal behind the derived bound of tests/test_gpu_frame_region.py."""
import numpy as np

INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def bw0(out_w, out_h):
    return max(1, min(1024 // max(min(16, out_h), 1), out_w))


def coords(M, out_w, out_h):
    """The fixed-point source coordinates X, Y (int64 [out_h, out_w], 1/32 steps) of every destination pixel."""
    M = np.asarray(M, np.float64).reshape(9)
    x = np.arange(out_w, dtype=np.int64)[None, :]
    y = np.arange(out_h, dtype=np.int64)[:, None].astype(np.float64)
    b = bw0(out_w, out_h)
    xb = ((x // b) * b).astype(np.float64)
    x1 = (x - (x // b) * b).astype(np.float64)
    # every product and sum is one numpy operation: rounded on its own
    X0 = (M[0] * xb + M[1] * y) + M[2]
    Y0 = (M[3] * xb + M[4] * y) + M[5]
    W0 = (M[6] * xb + M[7] * y) + M[8]
    W = W0 + M[6] * x1
    with np.errstate(divide="ignore"):
        W = np.where(W != 0.0, 32.0 / np.where(W != 0.0, W, 1.0), 0.0)
    fX = np.clip((X0 + M[0] * x1) * W, INT_MIN, INT_MAX)
    fY = np.clip((Y0 + M[3] * x1) * W, INT_MIN, INT_MAX)
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)


def rectify(img, M, out_w, out_h):
    """img uint8 [h, w, 3] -> R uint8 [out_h, out_w, 3]."""
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    X, Y = coords(M, out_w, out_h)
    sx, ax, sy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    I = img.astype(np.int64)
    ax, ay = ax[:, :, None], ay[:, :, None]
    acc = I[y0, x0] * ((32 - ax) * (32 - ay)) + I[y0, x1] * (ax * (32 - ay)) + I[y1, x0] * ((32 - ax) * ay) + I[y1, x1] * (ax * ay)
    return ((acc + 512) >> 10).astype(np.uint8)


def exact_coords(M, out_w, out_h):
    """The exact (float64, unquantised) source coordinate of every destination pixel: (M0 x + M1 y + M2) / (M6 x + M7 y + M8)."""
    M = np.asarray(M, np.float64).reshape(9)
    x = np.arange(out_w, dtype=np.float64)[None, :]
    y = np.arange(out_h, dtype=np.float64)[:, None]
    W = M[6] * x + M[7] * y + M[8]
    return (M[0] * x + M[1] * y + M[2]) / W, (M[3] * x + M[4] * y + M[5]) / W


def bilinear_f64(img, u, v):
    """Bilinear interpolation of img (replicate border) at the float64 coordinates u (x), v (y) -> float64 [.., 3]."""
    h, w, _ = img.shape
    I = img.astype(np.float64)
    fx, fy = np.floor(u), np.floor(v)
    a, b = (u - fx)[..., None], (v - fy)[..., None]
    x0 = np.clip(fx, 0, w - 1).astype(np.int64); x1 = np.clip(fx + 1, 0, w - 1).astype(np.int64)
    y0 = np.clip(fy, 0, h - 1).astype(np.int64); y1 = np.clip(fy + 1, 0, h - 1).astype(np.int64)
    return (I[y0, x0] * (1 - a) + I[y0, x1] * a) * (1 - b) + (I[y1, x0] * (1 - a) + I[y1, x1] * a) * b


def local_steps(img, u, v, r=2):
    """Dx, Dy per destination pixel: the largest absolute difference (any channel) between horizontally (vertically) adjacent
    source pixels within r pixels of the exact coordinate (u, v) — the pixels (px, py) with |px - u| <= r and |py - v| <= r, read
    under the replicate border."""
    h, w, _ = img.shape
    I = img.astype(np.int64)
    lx, hx = np.ceil(u - r).astype(np.int64), np.floor(u + r).astype(np.int64)
    ly, hy = np.ceil(v - r).astype(np.int64), np.floor(v + r).astype(np.int64)
    Dx = np.zeros(u.shape, np.int64); Dy = np.zeros(u.shape, np.int64)

    def at(py, px):
        return I[np.clip(py, 0, h - 1), np.clip(px, 0, w - 1)]
    for j in range(2 * r + 1):
        py = ly + j
        for k in range(2 * r + 1):
            px = lx + k
            inside = (py <= hy) & (px <= hx)
            dx = np.abs(at(py, px + 1) - at(py, px)).max(axis=-1)
            dy = np.abs(at(py + 1, px) - at(py, px)).max(axis=-1)
            Dx = np.maximum(Dx, np.where(inside & (px + 1 <= hx), dx, 0))
            Dy = np.maximum(Dy, np.where(inside & (py + 1 <= hy), dy, 0))
    return Dx, Dy
