"""The numpy restatement of include/slideo_amd.h "Frame pixel format", written from the header: which bytes of a frame under a
format are the B, G and R of pixel (x, y), the frame's span, the layouts and sizes the tests walk."""
import numpy as np

FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "argb": 4, "abgr": 5, "planar_rgb": 6, "planar_bgr": 7, "planar_gbr": 8}
NAMES = {v: k for k, v in FORMATS.items()}
C_NAMES = {0: "SLIDEO_PIXEL_BGR8", 1: "SLIDEO_PIXEL_RGB8", 2: "SLIDEO_PIXEL_BGRA8", 3: "SLIDEO_PIXEL_RGBA8", 4: "SLIDEO_PIXEL_ARGB8",
           5: "SLIDEO_PIXEL_ABGR8", 6: "SLIDEO_PIXEL_PLANAR_RGB8", 7: "SLIDEO_PIXEL_PLANAR_BGR8", 8: "SLIDEO_PIXEL_PLANAR_GBR8"}
NON_DEFAULT = [f for f in FORMATS if f != "bgr"]
# the order of a packed pixel's bytes / of a planar frame's planes ("x": ignored)
ORDER = {"bgr": "BGR", "rgb": "RGB", "bgra": "BGRx", "rgba": "RGBx", "argb": "xRGB", "abgr": "xBGR",
         "planar_rgb": "RGB", "planar_bgr": "BGR", "planar_gbr": "GBR"}


def _name(fmt):
    return NAMES[fmt] if not isinstance(fmt, str) else fmt


def info(fmt):
    """(bytes per pixel of a row, planes): 3 / 4 and 1 for packed formats, 1 and 3 for planar ones."""
    fmt = _name(fmt)
    if fmt.startswith("planar"):
        return 1, 3
    return len(ORDER[fmt]), 1


def span(fmt, w, h, stride):
    """bytes of one frame: height * stride_bytes, three times that for planar formats."""
    return info(fmt)[1] * h * stride


def to_bgr(buf, w, h, stride, fmt):
    """The BGR image (h, w, 3) a frame at buf (flat uint8) stands for: pixel (x, y) has the frame's B, G and R bytes of that pixel."""
    fmt = _name(fmt)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    bpp, planes = info(fmt)
    out = np.empty((h, w, 3), np.uint8)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for c, ch in enumerate("BGR"):
        k = ORDER[fmt].index(ch)
        idx = k * h * stride + ys * stride + xs if planes == 3 else ys * stride + xs * bpp + k
        out[:, :, c] = buf[idx]
    return out


def pack(bgr, fmt, stride=None, frame_bytes=None, seed=0):
    """The frame of `fmt` (flat uint8, frame_bytes long: at least the span) that stands for the image bgr (h, w, 3).  Row padding,
    the x bytes and the bytes behind the span are random: a kernel that reads them into the image is caught."""
    fmt = _name(fmt)
    h, w, _ = bgr.shape
    bpp, planes = info(fmt)
    stride = stride or w * bpp
    sp = span(fmt, w, h, stride)
    frame_bytes = frame_bytes or sp
    assert stride >= w * bpp and frame_bytes >= sp
    buf = np.random.default_rng(seed).integers(0, 256, frame_bytes, dtype=np.uint8)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for c, ch in enumerate("BGR"):
        k = ORDER[fmt].index(ch)
        idx = k * h * stride + ys * stride + xs if planes == 3 else ys * stride + xs * bpp + k
        buf[idx] = bgr[:, :, c]
    return buf


def as_array(buf, fmt, w, h):
    """A TIGHT frame (or n of them, [n, span]) in the array shape the Python frame methods take under fmt."""
    fmt = _name(fmt)
    bpp, planes = info(fmt)
    buf = np.asarray(buf, np.uint8)
    lead = buf.shape[:-1]
    return buf.reshape(lead + ((3, h, w) if planes == 3 else (h, w, bpp)))


def sizes():
    """(w, h): only ragged pixels; tails of 2 and 3; several threads; whole blocks; a width beyond one block's columns with a ragged end."""
    return [(1, 1), (2, 1), (3, 2), (6, 3), (7, 5), (34, 5), (64, 36), (4 * 64 * 2 + 6, 3)]


def layouts(fmt, w, h):
    """(name, stride) of fmt at w x h: tight, pitched at a multiple of 16, and one pitch per narrower load class — 8 mod 16,
    4 mod 8, 2 mod 4, odd.  (For a planar format with an odd number of rows the pitch of 2 mod 4 starts the second plane at an
    address that is 2 mod 4.)"""
    row = w * info(fmt)[0]
    up16 = -(-row // 16) * 16
    return [("tight", row), ("pitch16", up16 + 16), ("pitch8", up16 + 8), ("pitch4", up16 + 4), ("pitch2", up16 + 2), ("odd", up16 + 1)]
