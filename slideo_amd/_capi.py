"""ctypes binding of include/slideo_amd.h (libslideo_amd.so).

The product path.  It fails loudly when the HIP library is missing or no gfx950
device is present; there is no CPU fallback and nothing here imports oracle/.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

OK = 0
ERR_NAMES = {1: "INVALID_ARG", 2: "NO_DEVICE", 3: "HIP", 4: "STATE", 5: "UNSUPPORTED",
             6: "EMPTY_INDEX", 7: "CAPACITY"}


class OcvVariants(C.Structure):
    """slideo_ocv_variants (include/slideo_amd.h): which restatement of each OpenCV primitive runs."""
    _fields_ = [("gray", C.c_int32), ("blur", C.c_int32), ("resize", C.c_int32), ("atan", C.c_int32),
                ("warp", C.c_int32), ("area", C.c_int32), ("lm", C.c_int32), ("rng_mul", C.c_uint32),
                ("hdlt", C.c_int32)]


class Config(C.Structure):
    """slideo_config (include/slideo_amd.h); defaults = the reference's literals."""
    _fields_ = [
        ("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
        ("edge_threshold", C.c_int32), ("patch_size", C.c_int32), ("fast_threshold", C.c_int32),
        ("knn_k", C.c_int32), ("vote_tolerance", C.c_float), ("max_candidate_pages", C.c_int32),
        ("ransac_threshold", C.c_double), ("ransac_max_iters", C.c_int32),
        ("ransac_confidence", C.c_double), ("refine_iters", C.c_int32), ("max_rated", C.c_int32),
        ("min_rating", C.c_double), ("min_rating_ratio", C.c_double), ("min_similarity", C.c_float),
        ("small_area", C.c_int32), ("changed_similarity", C.c_float), ("ratio_test", C.c_float),
        ("verify_model", C.c_int32), ("matcher", C.c_int32), ("lsh_tables", C.c_int32), ("lsh_key_bits", C.c_int32),
        ("lsh_multi_probe", C.c_int32), ("verdict_rule", C.c_int32),
        ("ocv", OcvVariants),
    ]


class SiftConfig(C.Structure):
    """slideo_sift_config (include/slideo_amd.h): cv::SIFT::create's arguments."""
    _fields_ = [("nfeatures", C.c_int32), ("n_octave_layers", C.c_int32), ("contrast_threshold", C.c_double),
                ("edge_threshold", C.c_double), ("sigma", C.c_double)]


class Yuv420Layout(C.Structure):
    """slideo_yuv420_layout (include/slideo_amd.h, "YUV 4:2:0 frames"): where the planes of one decoded frame sit."""
    _fields_ = [("y_stride", C.c_int32), ("uv_stride", C.c_int32), ("u_offset", C.c_int64), ("v_offset", C.c_int64),
                ("uv_step", C.c_int32), ("_pad", C.c_int32)]


YUV420_FORMATS = {"nv12": 0, "nv21": 1, "i420": 2, "yv12": 3}


YUV_MATRICES = {"bt601": 0, "bt709": 1}
YUV_RANGES = {"limited": 0, "full": 1}
YUV_DEPTHS = {8: 0, "8": 0, "10_msb": 1, "p010": 1, "10_lsb": 2, "10le": 2}


def _yuv_enum(table, v, what):
    """A name of `table` (or the C value itself) -> the C value."""
    if isinstance(v, str) or (table is YUV_DEPTHS and v == 8):
        key = v.lower() if isinstance(v, str) else v
        if key not in table:
            raise SlideoError(1, "yuv description: unknown %s %r (one of %s)" % (what, v, sorted(map(str, table))))
        return table[key]
    return int(v)


def yuv_coefficients(matrix="bt601", range="limited"):
    """slideo_yuv_coefficients: (CY, CUB, CUG, CVG, CVR, y_offset, SHIFT) of the fixed-point conversion under (matrix, range)."""
    out = (C.c_int32 * 7)()
    rc = lib().slideo_yuv_coefficients(_yuv_enum(YUV_MATRICES, matrix, "matrix"), _yuv_enum(YUV_RANGES, range, "range"), out)
    if rc != OK:
        raise SlideoError(rc, "slideo_yuv_coefficients(%r, %r)" % (matrix, range))
    return tuple(int(v) for v in out)


def yuv420_layout(fmt, w, h, pitch=None, row_align=None, bytes_per_sample=1):
    """Layout of a `fmt` frame ('nv12', 'nv21', 'i420', 'yv12') of w x h -> (Yuv420Layout, frame bytes).  pitch: bytes per luma
    row (default w * bytes_per_sample; a planar format's chroma rows take pitch / 2); row_align: the chroma plane starts at
    pitch * align(h, row_align), as on a decoder surface.  Without either, the tightly packed layout (what
    slideo_yuv420_layout_packed / _packed16 returns).  bytes_per_sample=2: 16-bit containers ("YUV colour description")."""
    if fmt not in YUV420_FORMATS:
        raise ValueError("unknown 4:2:0 format %r" % (fmt,))
    if bytes_per_sample not in (1, 2):
        raise ValueError("bytes_per_sample is 1 or 2")
    p = int(pitch or w * bytes_per_sample)
    ah = -(-h // row_align) * row_align if row_align else h
    luma = p * ah
    L = Yuv420Layout()
    L.y_stride = p
    if fmt in ("nv12", "nv21"):
        L.uv_stride, L.uv_step = p, 2
        L.u_offset, L.v_offset = (luma, luma + bytes_per_sample) if fmt == "nv12" else (luma + bytes_per_sample, luma)
    else:
        L.uv_stride, L.uv_step = p // 2, 1
        first, second = luma, luma + (p // 2) * (ah // 2)
        L.u_offset, L.v_offset = (first, second) if fmt == "i420" else (second, first)
    return L, luma * 3 // 2


def yuv420_layout_packed(fmt, w, h, bytes_per_sample=1):
    """slideo_yuv420_layout_packed (bytes_per_sample=2: _packed16): the library's own tightly packed layout of `fmt`."""
    L = Yuv420Layout()
    name = "slideo_yuv420_layout_packed16" if bytes_per_sample == 2 else "slideo_yuv420_layout_packed"
    rc = getattr(lib(), name)(YUV420_FORMATS[fmt], int(w), int(h), C.byref(L))
    if rc != OK:
        raise SlideoError(rc, "%s(%s, %d, %d)" % (name, fmt, w, h))
    return L


# "YUV sampling": the formats of slideo_yuv_layout_packed (SLIDEO_YUV422_* / SLIDEO_YUV444_*) and the samplings
YUV_FORMATS = {"i422": 16, "yv16": 17, "nv16": 18, "nv61": 19, "yuy2": 20, "uyvy": 21, "yvyu": 22, "vyuy": 23,
               "i444": 24, "yv24": 25, "nv24": 26, "nv42": 27}
YUV_PACKED_OFFSETS = {"yuy2": (1, 3), "yvyu": (3, 1), "uyvy": (0, 2), "vyuy": (2, 0)}
YUV_SAMPLINGS = {"420": 0, "422": 1, "444": 2, "422_packed": 3}
# "YUV chroma filter": the SLIDEO_YUV_CHROMA_* values
YUV_CHROMA_FILTERS = {"nearest": 0, "left": 1, "center": 2, "topleft": 3}


def yuv_chroma_value(filt):
    """A name of YUV_CHROMA_FILTERS (or the SLIDEO_YUV_CHROMA_* value itself) -> the C value; ValueError for an unknown name or a
    value that is no integer."""
    if isinstance(filt, str):
        if filt.lower() not in YUV_CHROMA_FILTERS:
            raise ValueError("yuv chroma filter: unknown %r (one of %s)" % (filt, sorted(YUV_CHROMA_FILTERS)))
        return YUV_CHROMA_FILTERS[filt.lower()]
    if isinstance(filt, bool) or not isinstance(filt, (int, np.integer)):
        raise ValueError("yuv chroma filter: a name (one of %s) or a SLIDEO_YUV_CHROMA_* value, got %r" % (sorted(YUV_CHROMA_FILTERS), filt))
    return int(filt)


def yuv_chroma_weights(filt="left", sampling="420"):
    """slideo_yuv_chroma_weights: (wh, wv), each ((parity 0: k-1, k, k+1), (parity 1: ...)) in quarters, of the bilinear chroma
    filter `filt` under `sampling` (names or C values); an axis that is not interpolated is (0, 4, 0) twice."""
    if isinstance(sampling, str):
        if sampling.lower() not in YUV_SAMPLINGS:
            raise ValueError("yuv sampling: unknown %r (one of %s)" % (sampling, sorted(YUV_SAMPLINGS)))
        sampling = YUV_SAMPLINGS[sampling.lower()]
    out = (C.c_int32 * 12)()
    rc = lib().slideo_yuv_chroma_weights(yuv_chroma_value(filt), int(sampling), out)
    if rc != OK:
        raise SlideoError(rc, "slideo_yuv_chroma_weights(%r, %r)" % (filt, sampling))
    v = [int(x) for x in out]
    return (tuple(v[0:3]), tuple(v[3:6])), (tuple(v[6:9]), tuple(v[9:12]))


# "YUV transfer": the SLIDEO_YUV_TRANSFER_* values
YUV_TRANSFERS = {"sdr": 0, "hlg": 1, "pq": 2}


def yuv_transfer_value(transfer):
    """A name of YUV_TRANSFERS (or the SLIDEO_YUV_TRANSFER_* value itself) -> the C value; ValueError for an unknown name or a value
    that is no integer."""
    if isinstance(transfer, str):
        if transfer.lower() not in YUV_TRANSFERS:
            raise ValueError("yuv transfer: unknown %r (one of %s)" % (transfer, sorted(YUV_TRANSFERS)))
        return YUV_TRANSFERS[transfer.lower()]
    if isinstance(transfer, bool) or not isinstance(transfer, (int, np.integer)):
        raise ValueError("yuv transfer: a name (one of %s) or a SLIDEO_YUV_TRANSFER_* value, got %r" % (sorted(YUV_TRANSFERS), transfer))
    return int(transfer)


def yuv_transfer_tables(transfer="hlg", range_="limited", white_nits=0):
    """slideo_yuv_transfer_tables: the whole definition of "YUV transfer" as integers — (coef7 int32 [7]: CY, CUB, CUG, CVG, CVR,
    y_offset, SHIFT; gamut9 int32 [3, 3]; LIN uint16 [1024]; OUT uint8 [4096]) of (transfer, range, white_nits); names or C values.
    Pure host: no device is touched."""
    if isinstance(range_, str):
        if range_.lower() not in YUV_RANGES:
            raise ValueError("yuv range: unknown %r (one of %s)" % (range_, sorted(YUV_RANGES)))
        range_ = YUV_RANGES[range_.lower()]
    coef, gamut = np.zeros(7, np.int32), np.zeros((3, 3), np.int32)
    lin, out = np.zeros(1024, np.uint16), np.zeros(4096, np.uint8)
    rc = lib().slideo_yuv_transfer_tables(yuv_transfer_value(transfer), int(range_), C.c_float(white_nits), coef.ctypes.data, gamut.ctypes.data,
                                          lin.ctypes.data, out.ctypes.data)
    if rc != OK:
        raise SlideoError(rc, "slideo_yuv_transfer_tables(%r, %r, %r)" % (transfer, range_, white_nits))
    return coef, gamut, lin, out


# "Frame pixel format": the formats every *_bgr8 frame call can read its frames under (SLIDEO_PIXEL_*)
PIXEL_FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "argb": 4, "abgr": 5, "planar_rgb": 6, "planar_bgr": 7, "planar_gbr": 8}


def pixel_format_value(fmt):
    """The SLIDEO_PIXEL_* value of a name of PIXEL_FORMATS (or the value itself)."""
    if isinstance(fmt, str):
        if fmt.lower() not in PIXEL_FORMATS:
            raise SlideoError(1, "pixel format: unknown %r (one of %s)" % (fmt, sorted(PIXEL_FORMATS)))
        return PIXEL_FORMATS[fmt.lower()]
    return int(fmt)


def pixel_format_info(fmt):
    """slideo_pixel_format_info: (bytes per pixel of a row: 3, 4, or 1 for a plane's; planes: 1 or 3)."""
    bpp, planes = C.c_int32(), C.c_int32()
    if not hasattr(lib(), "slideo_pixel_format_info") and pixel_format_value(fmt) == 0:
        return 3, 1                                               # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
    rc = lib().slideo_pixel_format_info(pixel_format_value(fmt), C.byref(bpp), C.byref(planes))
    if rc != OK:
        raise SlideoError(rc, "slideo_pixel_format_info(%r)" % (fmt,))
    return bpp.value, planes.value


def _levels_table(lut):
    """A frame levels table as contiguous uint8 [3, 256] (B, G, R); ValueError for another shape, dtype or range."""
    a = np.asarray(lut)
    if a.shape not in ((3, 256), (768,)):
        raise ValueError("frame levels: expected a table of shape [3, 256] (B, G, R), got %s" % (a.shape,))
    if a.dtype != np.uint8:
        if not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 255:
            raise ValueError("frame levels: the table's entries are integers in 0..255")
    return np.ascontiguousarray(a.reshape(3, 256), np.uint8)


def _shading_field(aw, ah, cell, gains):
    """A frame shading as (aw, ah, cell, contiguous uint16 [gh + 1, gw + 1]); ValueError for another cell, shape, dtype or range."""
    aw, ah, cell = int(aw), int(ah), int(cell)
    if cell not in (16, 32, 64):
        raise ValueError("frame shading: cell %d is none of 16, 32, 64" % cell)
    if aw < 1 or ah < 1:
        raise ValueError("frame shading: analysed size %dx%d" % (aw, ah))
    gw, gh = -(-aw // cell), -(-ah // cell)
    a = np.asarray(gains)
    if a.shape not in ((gh + 1, gw + 1), ((gh + 1) * (gw + 1),)):
        raise ValueError("frame shading: expected gains of shape [%d, %d] (gh + 1, gw + 1), got %s" % (gh + 1, gw + 1, a.shape))
    if a.dtype != np.uint16:
        if not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() > 65535:
            raise ValueError("frame shading: the gains are integers in 1..65535 (Q8.8, 256 = 1.0)")
    if a.min() < 1:
        raise ValueError("frame shading: a gain of 0 (every gain is at least 1)")
    return aw, ah, cell, np.ascontiguousarray(a.reshape(gh + 1, gw + 1), np.uint16)


def shading_field(cnt, sum_f, sum_p, cell, min_count, min_gain, max_gain, smooth):
    """slideo_shading_field: the Q8.8 nodes uint16 [gh + 1, gw + 1] of per-cell sums cnt, sum_f, sum_p [gh, gw], and the number of
    valid cells.  min_gain, max_gain: Q8.8 integers.  SlideoError for what the header refuses."""
    cnt = np.ascontiguousarray(cnt, np.uint64)
    if cnt.ndim != 2:
        raise ValueError("shading_field: cnt is [gh, gw], got %s" % (cnt.shape,))
    gh, gw = cnt.shape
    sum_f, sum_p = np.ascontiguousarray(sum_f, np.uint64), np.ascontiguousarray(sum_p, np.uint64)
    if sum_f.shape != cnt.shape or sum_p.shape != cnt.shape:
        raise ValueError("shading_field: the three arrays share one shape")
    out, used = np.empty((gh + 1, gw + 1), np.uint16), C.c_int32()
    rc = lib().slideo_shading_field(_p(cnt), _p(sum_f), _p(sum_p), gw, gh, int(cell), C.c_int64(int(min_count)), int(min_gain), int(max_gain),
                                    int(smooth), _p(out), C.byref(used))
    if rc != OK:
        raise SlideoError(rc, "slideo_shading_field")
    return out, used.value


def frame_levels_lut(lo, hi):
    """slideo_frame_levels_lut: the stretch table uint8 [3, 256] (B, G, R) of the points lo, hi (three each, or one for all three):
    lut[c][x] = clamp(floor((510 (x - lo) + (hi - lo)) / (2 (hi - lo))), 0, 255).  ValueError unless 0 <= lo < hi <= 255."""
    lo3 = [int(v) for v in (lo if np.ndim(lo) else [lo] * 3)]
    hi3 = [int(v) for v in (hi if np.ndim(hi) else [hi] * 3)]
    if len(lo3) != 3 or len(hi3) != 3:
        raise ValueError("frame_levels_lut: three lo and three hi (B, G, R), got %d and %d" % (len(lo3), len(hi3)))
    for c in range(3):
        if not 0 <= lo3[c] < hi3[c] <= 255:
            raise ValueError("frame_levels_lut: channel %d has lo %d, hi %d: 0 <= lo < hi <= 255" % (c, lo3[c], hi3[c]))
    out = np.empty((3, 256), np.uint8)
    rc = lib().slideo_frame_levels_lut((C.c_int32 * 3)(*lo3), (C.c_int32 * 3)(*hi3), _p(out))
    if rc != OK:
        raise SlideoError(rc, lib().slideo_last_error(None).decode())
    return out


def yuv_format_sampling(fmt):
    """The sampling name a format is read under."""
    if fmt in YUV420_FORMATS:
        return "420"
    if fmt not in YUV_FORMATS:
        raise ValueError("unknown YUV format %r" % (fmt,))
    return "422_packed" if fmt in YUV_PACKED_OFFSETS else "444" if YUV_FORMATS[fmt] >= 24 else "422"


def yuv_layout(fmt, w, h, pitch=None, row_align=None, bytes_per_sample=1):
    """Layout of a `fmt` frame of w x h -> (Yuv420Layout, frame bytes): the four 4:2:0 names go to yuv420_layout; the twelve of
    "YUV sampling" ('i422', 'yv16', 'nv16', 'nv61', 'yuy2', 'uyvy', 'yvyu', 'vyuy', 'i444', 'yv24', 'nv24', 'nv42') are laid out
    here.  pitch: bytes per luma row (a packed format's one plane: default 2 w); planar 4:2:2 chroma rows take pitch / 2,
    interleaved 4:4:4 chroma rows 2 * pitch, the others pitch.  row_align: every plane has align(h, row_align) rows.  Without
    either, the tight layout slideo_yuv_layout_packed returns."""
    if fmt in YUV420_FORMATS:
        return yuv420_layout(fmt, w, h, pitch, row_align, bytes_per_sample)
    sampling = yuv_format_sampling(fmt)
    if bytes_per_sample not in (1, 2):
        raise ValueError("bytes_per_sample is 1 or 2")
    b = bytes_per_sample
    ah = -(-h // row_align) * row_align if row_align else h
    L = Yuv420Layout()
    if sampling == "422_packed":
        if b != 1:
            raise SlideoError(5, "packed 4:2:2 is 8-bit")
        p = int(pitch or 2 * w)
        L.y_stride = L.uv_stride = p
        L.uv_step = 4
        L.u_offset, L.v_offset = YUV_PACKED_OFFSETS[fmt]
        return L, p * ah
    p = int(pitch or w * b)
    luma = p * ah
    L.y_stride = p
    kind = (YUV_FORMATS[fmt] - 16) % 8 if sampling == "422" else YUV_FORMATS[fmt] - 24      # 0 U V planes, 1 V U planes, 2 U V pairs, 3 V U pairs
    if kind >= 2:
        cp = p if sampling == "422" else 2 * p
        L.uv_stride, L.uv_step = cp, 2
        L.u_offset, L.v_offset = (luma, luma + b) if kind == 2 else (luma + b, luma)
        return L, luma + cp * ah
    cp = p // 2 if sampling == "422" else p
    L.uv_stride, L.uv_step = cp, 1
    first, second = luma, luma + cp * ah
    L.u_offset, L.v_offset = (first, second) if kind == 0 else (second, first)
    return L, luma + 2 * cp * ah


def yuv_layout_packed(fmt, w, h, bytes_per_sample=1):
    """slideo_yuv_layout_packed: the library's own tight layout of a "YUV sampling" format."""
    L = Yuv420Layout()
    rc = lib().slideo_yuv_layout_packed(YUV_FORMATS[fmt], int(w), int(h), int(bytes_per_sample), C.byref(L))
    if rc != OK:
        raise SlideoError(rc, "slideo_yuv_layout_packed(%s, %d, %d, %d)" % (fmt, w, h, bytes_per_sample))
    return L


def _yuv_frames(frames, w, h, layout):
    """frames: uint8 [n, frame_bytes] (or one frame, 1-D), or little-endian uint16 samples (16-bit containers), read as their
    bytes -> (contiguous uint8 [n, frame_bytes], layout, frame stride in bytes).  A format NAME stands for its packed 8-bit layout."""
    frames = np.asarray(frames)
    if frames.dtype == np.uint16:
        frames = np.ascontiguousarray(frames, "<u2")
        frames = frames.view(np.uint8).reshape(frames.shape[:-1] + (frames.shape[-1] * 2,))
    frames = np.ascontiguousarray(frames, np.uint8)
    frames = frames.reshape(1 if frames.ndim == 1 else frames.shape[0], -1)
    if isinstance(layout, str):
        layout = yuv_layout(layout, w, h)[0]
    return frames, layout, frames.shape[1]


# ---- frame lists (include/slideo_amd.h "Frame lists") ---------------------------------------------------------------------------------
FRAME_LIST_BGR = 0
FRAME_LIST_YUV = 1
FRAME_LIST_DOORS = {"bgr": FRAME_LIST_BGR, "yuv": FRAME_LIST_YUV}


class FrameListRec(C.Structure):
    """slideo_frame_list (56 bytes)."""
    _fields_ = [("door", C.c_int32), ("on_device", C.c_int32), ("n_frames", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("uv_step", C.c_int32), ("stride", C.c_int64 * 3), ("planes", C.c_void_p)]


class FrameList:
    """A slideo_frame_list record with its `planes` array, and the frames themselves kept alive (frame_list builds it)."""

    def __init__(self, rec, table, keep):
        self.rec, self.table, self.keep = rec, table, keep

    n = property(lambda self: self.rec.n_frames)
    width = property(lambda self: self.rec.width)
    height = property(lambda self: self.rec.height)

    def ref(self):
        return C.cast(C.byref(self.rec), C.c_void_p)


def _plane_of(a):
    """(address, bytes between rows, on_device, bytes per element) of one plane: a numpy array or a tensor whose rows are contiguous."""
    if isinstance(a, np.ndarray):
        if a.ndim < 1 or any(a.strides[i] != a.strides[i + 1] * a.shape[i + 1] for i in range(1, a.ndim - 1)) or a.strides[-1] != a.itemsize:
            raise ValueError("frame_list: the rows of a plane must be contiguous (strides %s of shape %s)" % (a.strides, a.shape))
        return a.ctypes.data, (a.strides[0] if a.ndim > 1 else a.nbytes), False, a.itemsize
    if hasattr(a, "data_ptr"):                                     # a torch tensor, host or device
        es = a.element_size()
        if a.dim() < 1 or a.stride(-1) != 1 or any(a.stride(i) != a.stride(i + 1) * a.shape[i + 1] for i in range(1, a.dim() - 1)):
            raise ValueError("frame_list: the rows of a plane must be contiguous (strides %s of shape %s)" % (a.stride(), tuple(a.shape)))
        return a.data_ptr(), (a.stride(0) * es if a.dim() > 1 else a.numel() * es), bool(a.is_cuda), es
    raise TypeError("frame_list: a plane is a numpy array or a tensor, got %r" % type(a))


def frame_list(frames, door="bgr", width=None, height=None, chroma=None, planar=False, bps=None):
    """The record of a frame list from a sequence of frames, each a numpy array or a tensor (one plane) or a tuple of planes, all in
    host memory or all in device memory; the frames are kept alive by the returned FrameList.
      door "bgr", packed formats   a frame is [h, w, 3] or [h, w, 4]
      door "bgr", planar=True      a frame is [3, h, w], or a tuple of three [h, w] planes
      door "yuv", chroma None      a frame is (Y, U, V)
      door "yuv", chroma "uv"/"vu" a frame is (Y, C) with interleaved chroma in that order
      door "yuv", chroma "yuy2" .. a frame is one packed 4:2:2 plane [h, 2 w]
    width, height: needed through the YUV door (the BGR door reads them off the first frame).  Row strides come from the arrays and
    must agree between frames.  bps: the bytes per sample of interleaved chroma (default: the plane's element size, so uint8 arrays
    that hold 16-bit containers need bps=2)."""
    door_v = FRAME_LIST_DOORS[door] if isinstance(door, str) else int(door)
    frames = list(frames)
    n = len(frames)
    table = (C.c_void_p * max(3 * n, 1))()
    strides, on_dev, uv_step = None, None, 0
    for i, f in enumerate(frames):
        planes = list(f) if isinstance(f, (tuple, list)) else [f]
        if door_v == FRAME_LIST_BGR and planar and len(planes) == 1:
            planes = [planes[0][c] for c in range(3)]
        got = [_plane_of(p) for p in planes]
        addr = [g[0] for g in got] + [0] * (3 - len(got))
        st = [g[1] for g in got] + [0] * (3 - len(got))
        if door_v == FRAME_LIST_YUV:
            if chroma in ("uv", "vu"):
                if len(got) != 2:
                    raise ValueError("frame_list: interleaved chroma takes (Y, C) frames")
                bps = int(bps or got[1][3])
                addr = [addr[0], addr[1] + (bps if chroma == "vu" else 0), addr[1] + (bps if chroma == "uv" else 0)]
                st, uv_step = [st[0], st[1], st[1]], 2
            elif chroma is not None:
                if len(got) != 1:
                    raise ValueError("frame_list: packed 4:2:2 frames are one plane")
                u, v = YUV_PACKED_OFFSETS[chroma]
                addr, st, uv_step = [addr[0], addr[0] + u, addr[0] + v], [st[0]] * 3, 4
            else:
                if len(got) != 3:
                    raise ValueError("frame_list: planar YUV frames are (Y, U, V)")
                uv_step = 1
        elif i == 0 and width is None:
            shp = tuple(planes[0].shape)
            height, width = (shp[0], shp[1])
        if any(g[2] != got[0][2] for g in got) or (on_dev is not None and got[0][2] != on_dev):
            raise ValueError("frame_list: host and device memory in one list")
        on_dev = got[0][2]
        if strides is not None and st != strides:
            raise ValueError("frame_list: frame %d has row strides %s, frame 0 has %s (one stride per plane for the whole list)" % (i, st, strides))
        strides = st
        for k in range(3):
            table[3 * i + k] = addr[k] or None
    if width is None or height is None:
        raise ValueError("frame_list: width and height are needed")
    rec = FrameListRec(door_v, int(bool(on_dev)), n, int(width), int(height), uv_step, (C.c_int64 * 3)(*(strides or [0, 0, 0])),
                       C.cast(table, C.c_void_p))
    return FrameList(rec, table, frames)


def sift_config(**over):
    c = SiftConfig()
    lib().slideo_sift_config_default(C.byref(c))
    for k, v in over.items():
        setattr(c, k, v)
    return c


KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4")])
VERDICT_DTYPE = np.dtype([("page_idx", "<i4"), ("similarity", "<f4"), ("inliers", "<i4"),
                          ("n_keypoints", "<i4")])
CANDIDATE_DTYPE = np.dtype([("page_idx", "<i4"), ("n_votes", "<i4"), ("inliers", "<i4"),
                            ("survived", "<i4"), ("similarity", "<f4"), ("_pad", "<i4"),
                            ("transform", "<f8", (9,))])

PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p)

EXPORTS = [
    "slideo_abi_version", "slideo_matcher_use_sift", "slideo_matcher_max_in_flight", "slideo_config_default", "slideo_matcher_create", "slideo_matcher_destroy",
    "slideo_last_error", "slideo_matcher_add_pages_bgr8", "slideo_matcher_finalize_pages",
    "slideo_matcher_page_count", "slideo_matcher_descriptor_count", "slideo_matcher_get_page_features",
    "slideo_match_frames_bgr8", "slideo_match_frames_bgr8_dev", "slideo_changed_mask_bgr8",
    "slideo_matcher_set_progress", "slideo_orb_bgr8", "slideo_pyramid_level_bgr8",
    "slideo_knn_hamming", "slideo_knn_l2_u8", "slideo_small_image_bgr8", "slideo_last_frame_candidates",
    "slideo_matcher_set_profiling", "slideo_matcher_read_profile", "slideo_matcher_read_shader_clock", "slideo_matcher_set_knn_engine", "slideo_matcher_set_knn_exact_lists",
    "slideo_match_frames_submit_dev", "slideo_match_frames_collect", "slideo_match_frames_collect_dev",
    "slideo_matcher_add_page_features", "slideo_matcher_get_page_small", "slideo_l2_set_train", "slideo_l2_knn_dev",
    "slideo_matcher_unique_descriptor_count", "slideo_match_kept_frames", "slideo_host_register", "slideo_host_unregister",
    "slideo_sift_config_default", "slideo_sift_bgr8", "slideo_sift_frames_dev", "slideo_sift_layer_bgr8", "slideo_knn_lsh",
    "slideo_device_count", "slideo_device_list", "slideo_group_create", "slideo_group_destroy", "slideo_group_last_error", "slideo_group_device_count",
    "slideo_group_member", "slideo_group_set_progress", "slideo_group_use_sift", "slideo_group_add_pages_bgr8",
    "slideo_group_finalize_pages", "slideo_group_page_count", "slideo_group_descriptor_count", "slideo_group_match_frames_bgr8",
    "slideo_group_last_frame_candidates", "slideo_group_changed_mask_bgr8", "slideo_group_match_kept_frames",
    "slideo_yuv420_layout_packed", "slideo_match_frames_yuv420", "slideo_match_frames_yuv420_dev", "slideo_match_frames_submit_yuv420_dev",
    "slideo_changed_mask_yuv420", "slideo_yuv420_to_bgr8", "slideo_group_match_frames_yuv420", "slideo_group_changed_mask_yuv420",
    "slideo_matcher_create_page_set", "slideo_matcher_use_page_set", "slideo_matcher_release_page_set", "slideo_matcher_page_set_info",
    "slideo_group_create_page_set", "slideo_group_use_page_set", "slideo_group_release_page_set",
    "slideo_working_size", "slideo_matcher_set_working_size", "slideo_matcher_get_working_size", "slideo_group_set_working_size",
    "slideo_reduce_bgr8",
    "slideo_changed_ssd_threshold", "slideo_matcher_gate_reset", "slideo_matcher_gate_last_small",
    "slideo_match_changed_frames_bgr8", "slideo_match_changed_frames_yuv420", "slideo_match_changed_frames_bgr8_dev",
    "slideo_match_changed_frames_yuv420_dev", "slideo_match_changed_frames_submit_dev", "slideo_match_changed_frames_submit_yuv420_dev",
    "slideo_match_changed_frames_collect",
    "slideo_matcher_gate_reset_from_frame_bgr8", "slideo_matcher_gate_reset_from_frame_yuv420", "slideo_matcher_gate_reset_from_frame_bgr8_dev",
    "slideo_matcher_gate_reset_from_frame_yuv420_dev", "slideo_group_gate_reset", "slideo_group_gate_last_small",
    "slideo_group_match_changed_frames_bgr8", "slideo_group_match_changed_frames_yuv420",
    "slideo_matcher_set_frame_mask", "slideo_matcher_frame_mask_info", "slideo_group_set_frame_mask", "slideo_frame_mask_level",
    "slideo_matcher_set_frame_mask_scope", "slideo_matcher_frame_mask_scope", "slideo_group_set_frame_mask_scope",
    "slideo_changed_ssd_threshold_n", "slideo_frame_mask_small",
    "slideo_matcher_set_direct_similarity", "slideo_matcher_direct_similarity", "slideo_group_set_direct_similarity",
    "slideo_direct_ssd_threshold", "slideo_page_small_ssd",
    "slideo_matcher_set_direct_scope", "slideo_matcher_direct_scope", "slideo_group_set_direct_scope", "slideo_page_small_ssd_valid",
    "slideo_matcher_set_frame_region", "slideo_matcher_frame_region", "slideo_group_set_frame_region", "slideo_frame_region_from_quad",
    "slideo_rectify_bgr8",
    "slideo_matcher_set_yuv_description", "slideo_matcher_yuv_description", "slideo_group_set_yuv_description", "slideo_yuv_coefficients",
    "slideo_yuv420_layout_packed16",
    "slideo_matcher_set_yuv_sampling", "slideo_matcher_yuv_sampling", "slideo_group_set_yuv_sampling", "slideo_yuv_layout_packed",
    "slideo_matcher_set_yuv_chroma", "slideo_matcher_yuv_chroma", "slideo_group_set_yuv_chroma", "slideo_yuv_chroma_weights",
    "slideo_matcher_set_yuv_transfer", "slideo_matcher_yuv_transfer", "slideo_group_set_yuv_transfer", "slideo_yuv_transfer_tables",
    "slideo_matcher_set_pixel_format", "slideo_matcher_pixel_format", "slideo_group_set_pixel_format", "slideo_pixel_format_info",
    "slideo_pixels_to_bgr8",
    "slideo_matcher_set_frame_levels", "slideo_matcher_frame_levels", "slideo_group_set_frame_levels", "slideo_frame_levels_lut",
    "slideo_levels_bgr8", "slideo_matcher_levels_begin", "slideo_matcher_levels_end", "slideo_matcher_levels_info",
    "slideo_matcher_levels_histogram", "slideo_matcher_levels_points",
    "slideo_matcher_set_frame_shading", "slideo_matcher_frame_shading", "slideo_group_set_frame_shading", "slideo_shading_bgr8",
    "slideo_shading_field",
    "slideo_matcher_shading_begin", "slideo_matcher_shading_end", "slideo_matcher_shading_info", "slideo_matcher_shading_sums",
    "slideo_group_shading_begin", "slideo_group_shading_end", "slideo_group_shading_info", "slideo_group_shading_sums",
    "slideo_matcher_activity_begin", "slideo_matcher_activity_end", "slideo_matcher_observe_frames_bgr8", "slideo_matcher_observe_frames_yuv420",
    "slideo_matcher_observe_frames_bgr8_dev", "slideo_matcher_observe_frames_yuv420_dev", "slideo_matcher_activity_info",
    "slideo_matcher_activity_counts", "slideo_matcher_activity_mask",
    "slideo_matcher_content_begin", "slideo_matcher_content_end", "slideo_matcher_content_info", "slideo_matcher_content_counts",
    "slideo_matcher_content_box",
    "slideo_matcher_set_gate_reference", "slideo_matcher_gate_reference", "slideo_group_set_gate_reference", "slideo_small_gram_ssd",
    "slideo_matcher_set_gate_settle", "slideo_matcher_gate_settle", "slideo_group_set_gate_settle", "slideo_small_carried_ssd",
    "slideo_gate_settle_walk",
    "slideo_matcher_gate_state_bytes", "slideo_matcher_gate_state_export", "slideo_matcher_gate_state_import",
    "slideo_group_set_gate_order", "slideo_group_gate_order", "slideo_group_gate_state_export", "slideo_group_gate_state_import",
    "slideo_group_gate_chain_waited",
    "slideo_matcher_set_gate_memory", "slideo_matcher_gate_memory", "slideo_group_set_gate_memory", "slideo_matcher_last_gate_refs",
    "slideo_group_last_gate_refs", "slideo_matcher_gate_memory_entries", "slideo_matcher_gate_memory_small", "slideo_gate_recall_walk",
    "slideo_match_frames_features_bgr8",
    "slideo_matcher_evidence_begin", "slideo_matcher_evidence_end", "slideo_matcher_evidence_info", "slideo_matcher_evidence_counts",
    "slideo_group_evidence_begin", "slideo_group_evidence_end", "slideo_group_evidence_info", "slideo_group_evidence_counts",
    "slideo_evidence_mask", "slideo_evidence_box", "slideo_matcher_rng_stream_len",
    "slideo_matcher_tone_begin", "slideo_matcher_tone_end", "slideo_matcher_tone_info", "slideo_matcher_tone_counts",
    "slideo_group_tone_begin", "slideo_group_tone_end", "slideo_group_tone_info", "slideo_group_tone_counts", "slideo_tone_lut",
    "slideo_matcher_placement_begin", "slideo_matcher_placement_end", "slideo_matcher_placement_info", "slideo_matcher_placement_sums",
    "slideo_group_placement_begin", "slideo_group_placement_end", "slideo_group_placement_info", "slideo_group_placement_sums",
    "slideo_placement_quad",
    "slideo_matcher_set_frame_lens", "slideo_matcher_frame_lens", "slideo_group_set_frame_lens", "slideo_frame_lens_point",
    "slideo_undistort_bgr8", "slideo_placement_lens",
    "slideo_match_frames_list", "slideo_match_frames_submit_list", "slideo_match_changed_frames_list",
    "slideo_match_changed_frames_submit_list", "slideo_changed_mask_list", "slideo_matcher_observe_frames_list",
    "slideo_matcher_gate_reset_from_frame_list", "slideo_group_match_frames_list", "slideo_group_match_changed_frames_list",
    "slideo_group_changed_mask_list", "slideo_frame_list_to_bgr8",
]

# frame mask scope (include/slideo_amd.h "Frame mask scope")
MASK_DETECT = 1
MASK_GATE = 2
# direct look-up scope (include/slideo_amd.h "Direct look-up scope")
DIRECT_WHOLE = 0
DIRECT_VALID = 1
# gate reference (include/slideo_amd.h "Gate reference")
GATE_PREVIOUS = 0
GATE_ANCHOR = 1
GATE_REFERENCES = {"previous": GATE_PREVIOUS, "anchor": GATE_ANCHOR}
# group gate order (include/slideo_amd.h "Group gate order")
GROUP_GATE_HALO = 0
GROUP_GATE_CHAIN = 1
GROUP_GATE_ORDERS = {"halo": GROUP_GATE_HALO, "chain": GROUP_GATE_CHAIN}
# gate memory (include/slideo_amd.h "Gate memory"): the capacity's limit and the two refs that are no ordinal
GATE_MEMORY_MAX = 64
GATE_REF_RESET = -1
GATE_REF_DEFERRED = -2


def gate_deferred(changed, similarity, changed_similarity):
    """The deferred frames of a gated call under a gate settle (include/slideo_amd.h "Gate settle"): away from the anchor and not
    matched, changed == 0 && similarity < changed_similarity -> bool [n]."""
    changed = np.asarray(changed).astype(bool)
    return ~changed & (np.asarray(similarity, np.float32) < np.float32(changed_similarity))

_lib = None


class SlideoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("slideo_amd error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


def lib():
    """Loads libslideo_amd.so (building it in-tree if the sources are newer)."""
    global _lib
    if _lib is None:
        path = os.environ.get("SLIDEO_LIB_PATH") or _build.HIP_LIB      # (SLIDEO_LIB_PATH: an experiment build of the same sources)
        if path == _build.HIP_LIB and (not os.path.exists(path) or os.environ.get("SLIDEO_REBUILD")):
            path = _build.build_hip()
        if not os.path.exists(path):
            raise RuntimeError("libslideo_amd.so is missing and could not be built; the HIP "
                               "extension is required (no fallback path exists)")
        L = C.CDLL(path)
        L.slideo_abi_version.restype = C.c_uint32
        L.slideo_last_error.restype = C.c_char_p
        L.slideo_last_error.argtypes = [C.c_void_p]
        L.slideo_matcher_descriptor_count.restype = C.c_int64
        L.slideo_matcher_unique_descriptor_count.restype = C.c_int64
        L.slideo_matcher_descriptor_count.argtypes = [C.c_void_p]
        L.slideo_matcher_page_count.argtypes = [C.c_void_p]
        L.slideo_matcher_max_in_flight.argtypes = [C.c_void_p]
        L.slideo_matcher_destroy.argtypes = [C.c_void_p]
        L.slideo_matcher_destroy.restype = None
        L.slideo_group_last_error.restype = C.c_char_p
        L.slideo_group_last_error.argtypes = [C.c_void_p]
        L.slideo_group_destroy.argtypes = [C.c_void_p]
        L.slideo_group_destroy.restype = None
        L.slideo_group_member.restype = C.c_void_p
        L.slideo_group_member.argtypes = [C.c_void_p, C.c_int32]
        L.slideo_group_device_count.argtypes = [C.c_void_p]
        L.slideo_device_list.argtypes = [C.c_void_p, C.c_int32]
        L.slideo_group_page_count.argtypes = [C.c_void_p]
        L.slideo_group_descriptor_count.argtypes = [C.c_void_p]
        L.slideo_group_descriptor_count.restype = C.c_int64
        if hasattr(L, "slideo_changed_ssd_threshold"):             # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            L.slideo_changed_ssd_threshold.restype = C.c_int64
            L.slideo_changed_ssd_threshold.argtypes = [C.c_float, C.c_int32, C.c_int32]
        if hasattr(L, "slideo_group_match_changed_frames_bgr8"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_gate_reset_from_frame_bgr8.argtypes = [vp, vp, i32, i32, i32]
            L.slideo_matcher_gate_reset_from_frame_yuv420.argtypes = [vp, vp, i32, i32, vp]
            L.slideo_matcher_gate_reset_from_frame_bgr8_dev.argtypes = [vp, vp, i32, i32, i32, vp]
            L.slideo_matcher_gate_reset_from_frame_yuv420_dev.argtypes = [vp, vp, i32, i32, vp, vp]
            L.slideo_group_gate_reset.argtypes = [vp, vp, i32, i32]
            L.slideo_group_gate_last_small.argtypes = [vp, vp, i64, vp, vp]
            L.slideo_group_match_changed_frames_bgr8.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp, vp, vp]
            L.slideo_group_match_changed_frames_yuv420.argtypes = [vp, i32, vp, i32, i32, vp, i64, vp, vp, vp]
        if hasattr(L, "slideo_match_frames_list"):                 # ("Frame lists")
            vp, i64 = C.c_void_p, C.c_int64
            L.slideo_match_frames_list.argtypes = [vp, vp, vp, vp]
            L.slideo_match_frames_submit_list.argtypes = [vp, vp, vp, vp]
            L.slideo_match_changed_frames_list.argtypes = [vp, vp, vp, vp, vp, vp]
            L.slideo_match_changed_frames_submit_list.argtypes = [vp, vp, vp, vp]
            L.slideo_changed_mask_list.argtypes = [vp, vp, vp, vp, vp, vp]
            L.slideo_matcher_observe_frames_list.argtypes = [vp, vp, vp]
            L.slideo_matcher_gate_reset_from_frame_list.argtypes = [vp, vp, vp]
            L.slideo_group_match_frames_list.argtypes = [vp, vp, vp]
            L.slideo_group_match_changed_frames_list.argtypes = [vp, vp, vp, vp, vp]
            L.slideo_group_changed_mask_list.argtypes = [vp, vp, vp, vp, vp, vp]
            L.slideo_frame_list_to_bgr8.argtypes = [vp, vp, vp, i64]
        if hasattr(L, "slideo_matcher_set_frame_mask"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_set_frame_mask.argtypes = [vp, vp, i32, i32, i32]
            L.slideo_matcher_frame_mask_info.argtypes = [vp, vp, vp, vp]
            L.slideo_group_set_frame_mask.argtypes = [vp, vp, i32, i32, i32]
            L.slideo_frame_mask_level.argtypes = [vp, i32, vp, i64, vp, vp]
        if hasattr(L, "slideo_matcher_set_frame_mask_scope"):
            vp, u32, i64 = C.c_void_p, C.c_uint32, C.c_int64
            L.slideo_matcher_set_frame_mask_scope.argtypes = [vp, u32]
            L.slideo_matcher_frame_mask_scope.argtypes = [vp, vp]
            L.slideo_group_set_frame_mask_scope.argtypes = [vp, u32]
            L.slideo_changed_ssd_threshold_n.restype = i64
            L.slideo_changed_ssd_threshold_n.argtypes = [C.c_float, i64]
            L.slideo_frame_mask_small.argtypes = [vp, vp, i64, vp, vp, vp]
        if hasattr(L, "slideo_matcher_set_direct_similarity"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_set_direct_similarity.argtypes = [vp, C.c_float]
            L.slideo_matcher_direct_similarity.argtypes = [vp, vp]
            L.slideo_group_set_direct_similarity.argtypes = [vp, C.c_float]
            L.slideo_direct_ssd_threshold.restype = i64
            L.slideo_direct_ssd_threshold.argtypes = [C.c_float, i64]
            L.slideo_page_small_ssd.argtypes = [vp, vp, i32, i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_direct_scope"):
            vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
            L.slideo_matcher_set_direct_scope.argtypes = [vp, u32]
            L.slideo_matcher_direct_scope.argtypes = [vp, vp]
            L.slideo_group_set_direct_scope.argtypes = [vp, u32]
            L.slideo_page_small_ssd_valid.argtypes = [vp, vp, i32, i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_frame_region"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_set_frame_region.argtypes = [vp, i32, i32, vp, i32, i32]
            L.slideo_matcher_frame_region.argtypes = [vp, vp, vp, vp, vp, vp, vp]
            L.slideo_group_set_frame_region.argtypes = [vp, i32, i32, vp, i32, i32]
            L.slideo_frame_region_from_quad.argtypes = [vp, i32, i32, vp]
            L.slideo_rectify_bgr8.argtypes = [vp, vp, i32, i32, i32, vp, i64]
        if hasattr(L, "slideo_matcher_set_frame_lens"):
            vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
            L.slideo_matcher_set_frame_lens.argtypes = [vp, i32, i32] + [f64] * 5
            L.slideo_matcher_frame_lens.argtypes = [vp] * 9
            L.slideo_group_set_frame_lens.argtypes = [vp, i32, i32] + [f64] * 5
            L.slideo_frame_lens_point.argtypes = [f64] * 7 + [vp, vp]
            L.slideo_undistort_bgr8.argtypes = [vp, vp, i32, i32, i32, vp, i64]
            L.slideo_placement_lens.argtypes = [vp] * 5 + [i32] * 5 + [i64, f64, f64, f64, i32, f64, i32, i32] + [vp] * 5
        if hasattr(L, "slideo_matcher_set_yuv_description"):
            vp, i32 = C.c_void_p, C.c_int32
            L.slideo_matcher_set_yuv_description.argtypes = [vp, i32, i32, i32]
            L.slideo_matcher_yuv_description.argtypes = [vp, vp, vp, vp]
            L.slideo_group_set_yuv_description.argtypes = [vp, i32, i32, i32]
            L.slideo_yuv_coefficients.argtypes = [i32, i32, vp]
            L.slideo_yuv420_layout_packed16.argtypes = [i32, i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_yuv_sampling"):
            L.slideo_matcher_set_yuv_sampling.argtypes = [vp, i32]
            L.slideo_matcher_yuv_sampling.argtypes = [vp, vp]
            L.slideo_group_set_yuv_sampling.argtypes = [vp, i32]
        if hasattr(L, "slideo_matcher_set_yuv_chroma"):
            L.slideo_matcher_set_yuv_chroma.argtypes = [vp, i32]
            L.slideo_matcher_yuv_chroma.argtypes = [vp, vp]
            L.slideo_group_set_yuv_chroma.argtypes = [vp, i32]
            L.slideo_yuv_chroma_weights.argtypes = [i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_yuv_transfer"):
            L.slideo_matcher_set_yuv_transfer.argtypes = [vp, i32, C.c_float]
            L.slideo_matcher_yuv_transfer.argtypes = [vp, vp, vp]
            L.slideo_group_set_yuv_transfer.argtypes = [vp, i32, C.c_float]
            L.slideo_yuv_transfer_tables.argtypes = [i32, i32, C.c_float, vp, vp, vp, vp]
            L.slideo_yuv_layout_packed.argtypes = [i32, i32, i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_pixel_format"):
            L.slideo_matcher_set_pixel_format.argtypes = [vp, i32]
            L.slideo_matcher_pixel_format.argtypes = [vp, vp]
            L.slideo_group_set_pixel_format.argtypes = [vp, i32]
            L.slideo_pixel_format_info.argtypes = [i32, vp, vp]
            L.slideo_pixels_to_bgr8.argtypes = [vp, vp, i32, i32, i32, vp, C.c_int64]
        if hasattr(L, "slideo_matcher_activity_begin"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_activity_begin.argtypes = [vp, i32]
            L.slideo_matcher_activity_end.argtypes = [vp]
            L.slideo_matcher_observe_frames_bgr8.argtypes = [vp, i32, vp, i32, i32, i32, i64]
            L.slideo_matcher_observe_frames_yuv420.argtypes = [vp, i32, vp, i32, i32, vp, i64]
            L.slideo_matcher_observe_frames_bgr8_dev.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp]
            L.slideo_matcher_observe_frames_yuv420_dev.argtypes = [vp, i32, vp, i32, i32, vp, i64, vp]
            L.slideo_matcher_activity_info.argtypes = [vp, vp, vp, vp, vp]
            L.slideo_matcher_activity_counts.argtypes = [vp, vp, i64, vp, vp, vp]
            L.slideo_matcher_activity_mask.argtypes = [vp, i32, i32, vp, i64, vp, vp, vp, vp]
        if hasattr(L, "slideo_matcher_evidence_begin"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            for pre in ("slideo_matcher_", "slideo_group_"):
                getattr(L, pre + "evidence_begin").argtypes = [vp, i32, i32]
                getattr(L, pre + "evidence_end").argtypes = [vp]
                getattr(L, pre + "evidence_info").argtypes = [vp] * 9
                getattr(L, pre + "evidence_counts").argtypes = [vp, vp, vp, i64, vp, vp, vp, vp]
            L.slideo_evidence_mask.argtypes = [vp, vp, i32, i32, i32, i32, i32, i64, i32, i32, vp, i64]
            L.slideo_evidence_box.argtypes = [vp, vp, i32, i32, i32, i32, i32, i64, i32, vp]
            L.slideo_matcher_rng_stream_len.argtypes = [vp, vp]
        if hasattr(L, "slideo_matcher_tone_begin"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            for pre in ("slideo_matcher_", "slideo_group_"):
                getattr(L, pre + "tone_begin").argtypes = [vp, i32, i32, i32]
                getattr(L, pre + "tone_end").argtypes = [vp]
                getattr(L, pre + "tone_info").argtypes = [vp] * 5
                getattr(L, pre + "tone_counts").argtypes = [vp] * 5
            L.slideo_tone_lut.argtypes = [vp, vp, i64, vp]
        if hasattr(L, "slideo_matcher_placement_begin"):
            vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
            for pre in ("slideo_matcher_", "slideo_group_"):
                getattr(L, pre + "placement_begin").argtypes = [vp, i32, i32, f64]
                getattr(L, pre + "placement_end").argtypes = [vp]
                getattr(L, pre + "placement_info").argtypes = [vp] * 9
                getattr(L, pre + "placement_sums").argtypes = [vp] * 6 + [i64] + [vp] * 4
            L.slideo_placement_quad.argtypes = [vp] * 5 + [i32] * 5 + [i64, f64, i32] + [vp] * 4
        if hasattr(L, "slideo_matcher_content_begin"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_content_begin.argtypes = [vp, i32]
            L.slideo_matcher_content_end.argtypes = [vp]
            L.slideo_matcher_content_info.argtypes = [vp, vp, vp, vp, vp]
            L.slideo_matcher_content_counts.argtypes = [vp, vp, i64, vp, vp, vp]
            L.slideo_matcher_content_box.argtypes = [vp, i32, i32, vp, vp, vp, i64]
        if hasattr(L, "slideo_matcher_set_frame_levels"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_matcher_set_frame_levels.argtypes = [vp, vp]
            L.slideo_matcher_frame_levels.argtypes = [vp, vp, vp]
            L.slideo_group_set_frame_levels.argtypes = [vp, vp]
            L.slideo_frame_levels_lut.argtypes = [vp, vp, vp]
            L.slideo_levels_bgr8.argtypes = [vp, vp, i32, i32, i32, vp, i64]
            L.slideo_matcher_levels_begin.argtypes = [vp]
            L.slideo_matcher_levels_end.argtypes = [vp]
            L.slideo_matcher_levels_info.argtypes = [vp, vp, vp]
            L.slideo_matcher_levels_histogram.argtypes = [vp, vp]
            L.slideo_matcher_levels_points.argtypes = [vp, i32, i32, vp, vp]
        if hasattr(L, "slideo_matcher_set_frame_shading"):
            L.slideo_matcher_set_frame_shading.argtypes = [vp, i32, i32, i32, vp]
            L.slideo_matcher_frame_shading.argtypes = [vp, vp, i64, vp, vp, vp, vp]
            L.slideo_group_set_frame_shading.argtypes = [vp, i32, i32, i32, vp]
            L.slideo_shading_bgr8.argtypes = [vp, vp, i32, i32, i32, vp, i64]
            L.slideo_shading_field.argtypes = [vp, vp, vp, i32, i32, i32, i64, i32, i32, i32, vp, vp]
        if hasattr(L, "slideo_matcher_shading_begin"):
            for who in ("matcher", "group"):
                getattr(L, "slideo_%s_shading_begin" % who).argtypes = [vp, i32, i32, i32, i32]
                getattr(L, "slideo_%s_shading_end" % who).argtypes = [vp]
                getattr(L, "slideo_%s_shading_info" % who).argtypes = [vp] * 10
                getattr(L, "slideo_%s_shading_sums" % who).argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp]
        if hasattr(L, "slideo_matcher_set_gate_reference"):
            vp, i32, u32 = C.c_void_p, C.c_int32, C.c_uint32
            L.slideo_matcher_set_gate_reference.argtypes = [vp, u32]
            L.slideo_matcher_gate_reference.argtypes = [vp, vp]
            L.slideo_group_set_gate_reference.argtypes = [vp, u32]
            L.slideo_small_gram_ssd.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        if hasattr(L, "slideo_matcher_set_gate_settle"):
            vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
            L.slideo_matcher_set_gate_settle.argtypes = [vp, f32, i32]
            L.slideo_matcher_gate_settle.argtypes = [vp, vp, vp]
            L.slideo_group_set_gate_settle.argtypes = [vp, f32, i32]
            L.slideo_small_carried_ssd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
            L.slideo_gate_settle_walk.argtypes = [vp, vp, vp, vp, i32, i64, i64, i32, i32, i32, vp, vp, vp, vp]
        if hasattr(L, "slideo_group_set_gate_order"):
            vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
            L.slideo_matcher_gate_state_bytes.argtypes = [vp, vp]
            L.slideo_matcher_gate_state_export.argtypes = [vp, vp, i64, vp]
            L.slideo_matcher_gate_state_import.argtypes = [vp, vp, i64]
            L.slideo_group_set_gate_order.argtypes = [vp, u32]
            L.slideo_group_gate_order.argtypes = [vp, vp]
            L.slideo_group_gate_state_export.argtypes = [vp, vp, i64, vp]
            L.slideo_group_gate_state_import.argtypes = [vp, vp, i64]
            L.slideo_group_gate_chain_waited.argtypes = [vp, i32, vp]
        if hasattr(L, "slideo_matcher_set_gate_memory"):
            vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
            L.slideo_matcher_set_gate_memory.argtypes = [vp, i32]
            L.slideo_matcher_gate_memory.argtypes = [vp, vp]
            L.slideo_group_set_gate_memory.argtypes = [vp, i32]
            L.slideo_matcher_last_gate_refs.argtypes = [vp, vp, i64, vp]
            L.slideo_group_last_gate_refs.argtypes = [vp, vp, i64, vp]
            L.slideo_matcher_gate_memory_entries.argtypes = [vp, vp, vp, vp]
            L.slideo_matcher_gate_memory_small.argtypes = [vp, i32, vp, i64, vp, vp]
            L.slideo_gate_recall_walk.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, u64, i32, i32, i64, i64, i32, i32, i32, i64,
                                                  vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "slideo_match_frames_features_bgr8"):
            vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
            L.slideo_match_frames_features_bgr8.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp, vp, vp, vp]
        _lib = L
    return _lib


def default_config(**over):
    c = Config()
    lib().slideo_config_default(C.byref(c))
    for k, v in over.items():
        tgt, name = (c.ocv, k[4:]) if k.startswith("ocv_") else (c, k)     # ocv_blur=2 -> c.ocv.blur = 2
        if not hasattr(tgt, name):
            raise AttributeError(k)
        setattr(tgt, name, v)
    return c


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _img3(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected an HxWx3 uint8 BGR image")
    return a


class _FrameCalls:
    """The host frame calls a Matcher and a Group share: the same C entry points under the symbol prefix _PREFIX ("slideo_" /
    "slideo_group_"), failures raised through the class's own _check."""
    _PREFIX = None

    def _call(self, name, *args):
        self._check(getattr(lib(), self._PREFIX + name)(self._h, *args))

    def _pix_frames(self, frames, what="frames"):
        """Host frames in the array shape of the pixel format in force ("Frame pixel format") — [n, h, w, 3], [n, h, w, 4] or
        [n, 3, h, w] — -> (the contiguous array, n, w, h, stride_bytes, frame_stride_bytes)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        fmt = self.pixel_format()
        bpp, planes = pixel_format_info(fmt)
        name = {v: k for k, v in PIXEL_FORMATS.items()}[fmt]
        if planes == 3:
            if frames.ndim != 4 or frames.shape[1] != 3:
                raise ValueError("%s: expected uint8 [n, 3, h, w] under the pixel format %r, got %s" % (what, name, frames.shape))
            n, _, h, w = frames.shape
            return frames, n, w, h, w, 3 * w * h
        if frames.ndim != 4 or frames.shape[3] != bpp:
            raise ValueError("%s: expected uint8 [n, h, w, %d] under the pixel format %r, got %s" % (what, bpp, name, frames.shape))
        n, h, w, _ = frames.shape
        return frames, n, w, h, w * bpp, w * h * bpp

    def _pix_strides(self, w, h, stride, frame_stride):
        """The default stride_bytes / frame_stride_bytes of tightly packed device frames under the pixel format in force."""
        bpp, planes = pixel_format_info(self.pixel_format())
        stride = stride or w * bpp
        return stride, frame_stride or planes * stride * h

    def _separate(self, frames):
        """A list or tuple of separate host frames in the array shape of the pixel format in force -> their FrameList ("Frame
        lists": no copy into one batch); anything else -> None (the contiguous call)."""
        if not isinstance(frames, (list, tuple)) or not frames or not all(isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.ndim == 3 for f in frames):
            return None
        bpp, planes = pixel_format_info(self.pixel_format())
        if any(f.shape != frames[0].shape or (f.shape[0] != 3 if planes == 3 else f.shape[2] != bpp) for f in frames):
            return None
        return frame_list([np.ascontiguousarray(f) for f in frames], "bgr", planar=planes == 3)

    def match_frames(self, frames):
        """frames: uint8 [n, h, w, 3] in host memory (the array shape of the pixel format in force) -> verdict records.  A list of
        separate frame arrays goes as a frame list."""
        fl = self._separate(frames)
        if fl is not None:
            return self.match_frames_list(fl)
        frames, n, w, h, st, fs = self._pix_frames(frames, "match_frames")
        out = np.zeros(n, VERDICT_DTYPE)
        self._call("match_frames_bgr8", n, _p(frames), w, h, st, C.c_int64(fs), _p(out))
        return out

    # ---- match evidence map (include/slideo_amd.h "Match evidence map"); a Group's are the members' sums ----
    def evidence_begin(self, cell, min_inliers):
        """An empty evidence session: match calls from now on count, per cell x cell cell of the analysed image, the keypoints of the
        frames whose verdict has a page and at least min_inliers inliers (seen), and those the winner's transform explains (hit)."""
        self._check(getattr(lib(), self._SETS + "evidence_begin")(self._h, int(cell), int(min_inliers)))

    def evidence_end(self):
        self._check(getattr(lib(), self._SETS + "evidence_end")(self._h))

    def evidence_info(self):
        """-> {cell, min_inliers, aw, ah, gw, gh, frames_through, frames_counted} (aw == 0 before the first counted call)."""
        v = [C.c_int32() for _ in range(6)] + [C.c_int64(), C.c_int64()]
        self._check(getattr(lib(), self._SETS + "evidence_info")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("cell", "min_inliers", "aw", "ah", "gw", "gh", "frames_through", "frames_counted"), (x.value for x in v)))

    def evidence_counts(self):
        """-> (seen uint32 [gh, gw], hit uint32 [gh, gw], frames_through, frames_counted); [0, 0] arrays before the first counted call."""
        gw, gh, ft, fc = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        fn = getattr(lib(), self._SETS + "evidence_counts")
        self._check(fn(self._h, None, None, C.c_int64(0), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        seen, hit = np.zeros((gh.value, gw.value), np.uint32), np.zeros((gh.value, gw.value), np.uint32)
        if seen.size:
            self._check(fn(self._h, _p(seen), _p(hit), C.c_int64(seen.size), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        return seen, hit, ft.value, fc.value

    # ---- match tone table (include/slideo_amd.h "Match tone table"); a Group's are the members' sums ----
    def tone_begin(self, min_inliers, min_hits, flat):
        """An empty tone session: match calls from now on count, per channel and frame value, the page values of the small-image
        pixels that the contributing candidate's hits enclose (the candidate with a model and the most inliers, at least min_inliers;
        at least min_hits hits; small-image pixels whose neighbours differ by at most flat)."""
        self._check(getattr(lib(), self._SETS + "tone_begin")(self._h, int(min_inliers), int(min_hits), int(flat)))

    def tone_end(self):
        self._check(getattr(lib(), self._SETS + "tone_end")(self._h))

    def tone_info(self):
        """-> {min_inliers, min_hits, flat, frames_through}."""
        v = [C.c_int32() for _ in range(3)] + [C.c_int64()]
        self._check(getattr(lib(), self._SETS + "tone_info")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("min_inliers", "min_hits", "flat", "frames_through"), (x.value for x in v)))

    def tone_counts(self):
        """-> (cnt uint64 [3, 256], sum uint64 [3, 256], frames_through, frames_counted)."""
        cnt, sm = np.zeros((3, 256), np.uint64), np.zeros((3, 256), np.uint64)
        ft, fc = C.c_int64(), C.c_int64()
        self._check(getattr(lib(), self._SETS + "tone_counts")(self._h, _p(cnt), _p(sm), C.byref(ft), C.byref(fc)))
        return cnt, sm, ft.value, fc.value

    # ---- match placement map (include/slideo_amd.h "Match placement map"); a Group's are the members' sums ----
    def placement_begin(self, cell, min_inliers, reach):
        """An empty placement session: match calls from now on sum, per cell x cell cell of the analysed image, the frame positions of
        the keypoints that the contributing candidate (a model, the most inliers, at least min_inliers) explains within `reach`
        pixels, and the unit-slide positions of their page points."""
        self._check(getattr(lib(), self._SETS + "placement_begin")(self._h, int(cell), int(min_inliers), C.c_double(float(reach))))

    def placement_end(self):
        self._check(getattr(lib(), self._SETS + "placement_end")(self._h))

    def placement_info(self):
        """-> {cell, min_inliers, reach, aw, ah, gw, gh, frames_through} (aw == 0 before the first counted call)."""
        v = [C.c_int32(), C.c_int32(), C.c_double()] + [C.c_int32() for _ in range(4)] + [C.c_int64()]
        self._check(getattr(lib(), self._SETS + "placement_info")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("cell", "min_inliers", "reach", "aw", "ah", "gw", "gh", "frames_through"), (x.value for x in v)))

    def placement_sums(self):
        """-> (sums uint64 [5, gh, gw]: n, sfx, sfy, su, sv; frames_through, frames_counted); [5, 0, 0] before the first counted call."""
        gw, gh, ft, fc = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        fn = getattr(lib(), self._SETS + "placement_sums")
        self._check(fn(self._h, None, None, None, None, None, C.c_int64(0), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        sums = np.zeros((5, gh.value, gw.value), np.uint64)
        if sums.size:
            self._check(fn(self._h, *[_p(sums[i]) for i in range(5)], C.c_int64(sums[0].size), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        return sums, ft.value, fc.value

    # ---- match shading map (include/slideo_amd.h "Match shading map"); a Group's are the members' sums ----
    def shading_begin(self, cell, min_inliers, min_hits, flat):
        """An empty shading session: match calls from now on sum, per cell x cell cell of the analysed image, the samples of the tone
        table's sampler that land there, their frame pixels' B + G + R and their page small-image pixels' B + G + R.  Refused while a
        frame shading or a frame levels table is set."""
        self._check(getattr(lib(), self._SETS + "shading_begin")(self._h, int(cell), int(min_inliers), int(min_hits), int(flat)))

    def shading_end(self):
        self._check(getattr(lib(), self._SETS + "shading_end")(self._h))

    def shading_info(self):
        """-> {cell, min_inliers, min_hits, flat, aw, ah, gw, gh, frames_through} (aw == 0 before the first counted call)."""
        v = [C.c_int32() for _ in range(8)] + [C.c_int64()]
        self._check(getattr(lib(), self._SETS + "shading_info")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("cell", "min_inliers", "min_hits", "flat", "aw", "ah", "gw", "gh", "frames_through"), (x.value for x in v)))

    def shading_sums(self):
        """-> (sums uint64 [3, gh, gw]: cnt, sum_f, sum_p; frames_through, frames_counted); [3, 0, 0] before the first counted call."""
        gw, gh, ft, fc = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        fn = getattr(lib(), self._SETS + "shading_sums")
        self._check(fn(self._h, None, None, None, C.c_int64(0), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        sums = np.zeros((3, gh.value, gw.value), np.uint64)
        if sums.size:
            self._check(fn(self._h, *[_p(sums[i]) for i in range(3)], C.c_int64(sums[0].size), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)))
        return sums, ft.value, fc.value

    def last_candidates(self, frame_in_batch):
        cands = np.zeros(64, CANDIDATE_DTYPE)
        n = C.c_int32()
        self._call("last_frame_candidates", frame_in_batch, _p(cands), 64, C.byref(n))
        return cands[: n.value].copy()

    def changed_mask(self, frames, prev_small=None):
        fl = self._separate(frames)
        if fl is not None:
            return self.changed_mask_list(fl, prev_small)
        frames, n, w, h, st, fs = self._pix_frames(frames, "changed_mask")
        return self._mask("changed_mask_bgr8", n, w, h, prev_small, _p(frames), w, h, st, C.c_int64(fs))

    # YUV 4:2:0 frames (include/slideo_amd.h "YUV 4:2:0 frames"): uint8 [n, frame_bytes] in host memory; layout: a Yuv420Layout
    # or a format name (its packed layout)
    def match_frames_yuv420(self, frames, w, h, layout="nv12"):
        frames, layout, fs = _yuv_frames(frames, w, h, layout)
        out = np.zeros(frames.shape[0], VERDICT_DTYPE)
        self._call("match_frames_yuv420", frames.shape[0], _p(frames), w, h, C.byref(layout), C.c_int64(fs), _p(out))
        return out

    def changed_mask_yuv420(self, frames, w, h, layout="nv12", prev_small=None):
        frames, layout, fs = _yuv_frames(frames, w, h, layout)
        return self._mask("changed_mask_yuv420", frames.shape[0], w, h, prev_small, _p(frames), w, h, C.byref(layout), C.c_int64(fs))

    def _mask(self, name, n, w, h, prev_small, *frame_args):
        """-> (changed [n] bool, similarity [n] f32, the last frame's small image)"""
        changed = np.zeros(n, np.uint8)
        sims = np.zeros(n, np.float32)
        sw, sh = small_size(*self._unit_size(w, h), self.cfg.small_area)
        last = np.zeros((sh, sw, 3), np.uint8)
        if prev_small is not None:
            prev_small = np.ascontiguousarray(prev_small, np.uint8)
        self._call(name, n, *frame_args, _p(prev_small), _p(last), _p(changed), _p(sims))
        return changed.astype(bool), sims, last

    # ---- frame lists (include/slideo_amd.h "Frame lists"): fl is a FrameList (frame_list); a Group takes host lists -------------
    def _list_stream(self, stream):
        return () if self._PREFIX == "slideo_group_" else (C.c_void_p(stream or None),)

    def match_frames_list(self, fl, stream=0):
        out = np.zeros(fl.n, VERDICT_DTYPE)
        self._call("match_frames_list", fl.ref(), _p(out), *self._list_stream(stream))
        return out

    def match_changed_frames_list(self, fl, stream=0):
        ch, sim, out = self._gated_out(fl.n)
        self._call("match_changed_frames_list", fl.ref(), _p(ch), _p(sim), _p(out), *self._list_stream(stream))
        return ch.astype(bool), sim, out

    def changed_mask_list(self, fl, prev_small=None):
        """-> (changed [n] bool, similarity [n] f32, the last frame's small image); match_kept_frames follows as it does changed_mask."""
        changed, sims = np.zeros(fl.n, np.uint8), np.zeros(fl.n, np.float32)
        sw, sh = small_size(*self._unit_size(fl.width, fl.height), self.cfg.small_area)
        last = np.zeros((sh, sw, 3), np.uint8)
        if prev_small is not None:
            prev_small = np.ascontiguousarray(prev_small, np.uint8)
        self._call("changed_mask_list", fl.ref(), _p(prev_small), _p(last), _p(changed), _p(sims))
        return changed.astype(bool), sims, last

    def match_kept_frames(self, sel):
        """Verdicts of frames `sel` (indices) of the LAST changed_mask call, from the copy that call left on the device."""
        sel = np.ascontiguousarray(sel, np.int32)
        out = np.zeros(len(sel), VERDICT_DTYPE)
        self._call("match_kept_frames", len(sel), _p(sel), _p(out))
        return out

    # ---- changed-frame gate (include/slideo_amd.h "Changed-frame gate"): the host forms a Matcher and a Group share -------------
    # Gated calls return (changed [n] bool, similarity [n] f32, verdicts [n]); an unchanged frame's verdict is (-1, 0, 0, 0).
    # A Group carries ONE gate state and returns what a single Matcher returns for the same sequence of calls.
    def gate_reset(self, prev_small=None):
        """The gate state: the small image (sh, sw, 3) the next gated frame compares against, or None (that frame is changed)."""
        if prev_small is None:
            self._check(getattr(lib(), self._SETS + "gate_reset")(self._h, None, 0, 0))
            return
        prev_small = np.ascontiguousarray(prev_small, np.uint8)
        if prev_small.ndim != 3 or prev_small.shape[2] != 3:
            raise SlideoError(1, "gate_reset: expected an (sh, sw, 3) uint8 small image")
        self._check(getattr(lib(), self._SETS + "gate_reset")(self._h, _p(prev_small), prev_small.shape[1], prev_small.shape[0]))

    def gate_last_small(self):
        """The small image of the last gated frame (SLIDEO_ERR_STATE when no frame was gated since a reset to None)."""
        sw, sh = C.c_int32(), C.c_int32()
        self._check(getattr(lib(), self._SETS + "gate_last_small")(self._h, None, C.c_int64(1 << 40), C.byref(sw), C.byref(sh)))
        out = np.empty((sh.value, sw.value, 3), np.uint8)
        self._check(getattr(lib(), self._SETS + "gate_last_small")(self._h, _p(out), C.c_int64(out.size), C.byref(sw), C.byref(sh)))
        return out

    def gate_state_export(self):
        """The whole gate state as a record (include/slideo_amd.h "Gate state record") -> bytes."""
        n = C.c_int64()
        rc = getattr(lib(), self._SETS + "gate_state_export")(self._h, None, C.c_int64(0), C.byref(n))
        if rc != 7:                                               # (SLIDEO_ERR_CAPACITY with the size set: the probe's answer)
            self._check(rc)
        out = np.zeros(max(int(n.value), 1), np.uint8)
        self._check(getattr(lib(), self._SETS + "gate_state_export")(self._h, _p(out), C.c_int64(out.size), C.byref(n)))
        return out[: n.value].tobytes()

    def gate_state_import(self, rec):
        """The gate state from a record of gate_state_export: every later gated call returns what the exporting matcher's would."""
        buf = np.frombuffer(bytes(rec), np.uint8)
        self._check(getattr(lib(), self._SETS + "gate_state_import")(self._h, _p(buf) if buf.size else None, C.c_int64(buf.size)))

    @staticmethod
    def _gated_out(n):
        return np.zeros(n, np.uint8), np.zeros(n, np.float32), np.zeros(n, VERDICT_DTYPE)

    def match_changed_frames(self, frames):
        """frames: uint8 [n, h, w, 3] in host memory, continuing the gate.  A list of separate frame arrays goes as a frame list."""
        fl = self._separate(frames)
        if fl is not None:
            return self.match_changed_frames_list(fl)
        frames, n, w, h, st, fs = self._pix_frames(frames, "match_changed_frames")
        ch, sim, out = self._gated_out(n)
        self._call("match_changed_frames_bgr8", n, _p(frames), w, h, st, C.c_int64(fs), _p(ch), _p(sim), _p(out))
        return ch.astype(bool), sim, out

    def match_changed_frames_yuv420(self, frames, w, h, layout="nv12"):
        frames, layout, fs = _yuv_frames(frames, w, h, layout)
        n = frames.shape[0]
        ch, sim, out = self._gated_out(n)
        self._call("match_changed_frames_yuv420", n, _p(frames), w, h, C.byref(layout), C.c_int64(fs), _p(ch), _p(sim), _p(out))
        return ch.astype(bool), sim, out

    # working size (include/slideo_amd.h "Working size"): frames beyond it stand for their INTER_AREA reduction
    def set_working_size(self, max_w, max_h):
        """Frames larger than max_w x max_h are reduced on the GPU before matching ((0, 0): none).  The matcher must be idle."""
        self._check(getattr(lib(), self._SETS + "set_working_size")(self._h, int(max_w), int(max_h)))
        self._ws = (int(max_w), int(max_h))

    @property
    def working_size(self):
        return getattr(self, "_ws", (0, 0))

    # frame mask (include/slideo_amd.h "Frame mask"): ORB keypoints of frames of the mask's size are detected under it
    def set_frame_mask(self, mask):
        """mask: uint8 [h, w], nonzero = detect here; None clears it.  Detection only; pages are never masked.  The matcher must
        be idle; frames of another analysed size are then an error (SLIDEO_ERR_INVALID_ARG)."""
        if mask is None:
            self._check(getattr(lib(), self._SETS + "set_frame_mask")(self._h, None, 0, 0, 0))
            return
        mask = np.ascontiguousarray(mask)
        if mask.ndim != 2 or mask.dtype != np.uint8:
            raise SlideoError(1, "set_frame_mask: expected an (h, w) uint8 mask")
        self._check(getattr(lib(), self._SETS + "set_frame_mask")(self._h, _p(mask), mask.shape[1], mask.shape[0], mask.shape[1]))

    # frame mask scope (include/slideo_amd.h "Frame mask scope"): which stages the frame mask applies to
    def set_frame_mask_scope(self, scope):
        """scope: MASK_DETECT (the default), MASK_GATE or both.  Under MASK_GATE the changed-frame flags and similarities ignore the
        masked regions.  The matcher's own: it survives clearing or replacing the mask.  The matcher must be idle."""
        self._check(getattr(lib(), self._SETS + "set_frame_mask_scope")(self._h, int(scope)))

    # direct page look-up (include/slideo_amd.h "Direct page look-up"): gated calls resolve full-screen slide frames without ORB
    def set_direct_similarity(self, t):
        """t: 0 (off, the default) or 0 < t <= 1.  While t > 0 a changed frame of a gated call whose small image is at least that
        similar to an eligible page's gets the verdict (page, similarity, 0 inliers, 0 keypoints) without the pipeline.  The
        matcher must be idle."""
        self._check(getattr(lib(), self._SETS + "set_direct_similarity")(self._h, C.c_float(t)))

    @property
    def direct_similarity(self):
        t = C.c_float()
        rc = lib().slideo_matcher_direct_similarity(self._mask_owner(), C.byref(t))
        if rc != OK:
            raise SlideoError(rc, "direct_similarity")
        return float(t.value)

    # direct look-up scope (include/slideo_amd.h "Direct look-up scope"): what the look-up compares
    def set_direct_scope(self, scope):
        """scope: DIRECT_WHOLE (the default: whole small images, refused beside MASK_GATE) or DIRECT_VALID (the valid pixels of the
        gate's validity map while a mask is set under MASK_GATE).  The matcher must be idle."""
        self._check(getattr(lib(), self._SETS + "set_direct_scope")(self._h, int(scope)))

    @property
    def direct_scope(self):
        scope = C.c_uint32()
        rc = lib().slideo_matcher_direct_scope(self._mask_owner(), C.byref(scope))
        if rc != OK:
            raise SlideoError(rc, "direct_scope")
        return scope.value

    # gate reference (include/slideo_amd.h "Gate reference"): which frame a gated frame is compared with
    def set_gate_reference(self, ref):
        """ref: 'previous' (the default: the frame before, MarkSimilarIter) or 'anchor' (the last frame that was flagged), or the
        SLIDEO_GATE_* value.  The matcher must be idle; resets the gate state.  A Group of more than one member refuses 'anchor'."""
        if isinstance(ref, str):
            if ref not in GATE_REFERENCES:
                raise SlideoError(1, "gate reference %r: 'previous' or 'anchor'" % (ref,))
            ref = GATE_REFERENCES[ref]
        self._check(getattr(lib(), self._SETS + "set_gate_reference")(self._h, int(ref)))

    def gate_reference(self):
        """'previous' or 'anchor' (a Group: member 0's)."""
        ref = C.c_uint32()
        rc = lib().slideo_matcher_gate_reference(self._mask_owner(), C.byref(ref))
        if rc != OK:
            raise SlideoError(rc, "gate_reference")
        return {v: k for k, v in GATE_REFERENCES.items()}[ref.value]

    # gate settle (include/slideo_amd.h "Gate settle"): under 'anchor', match a changed frame only once the picture stands still
    def set_gate_settle(self, similarity, max_defer):
        """similarity: 0 (off, the default) or 0 < s <= 1: a frame away from the anchor is matched once it is within s of the frame
        before it, or after max_defer (0 .. 2**31 - 1) deferred frames.  Needs the gate reference 'anchor'; the matcher must be idle;
        resets the gate state.  A Group of more than one member refuses a settle that is on."""
        max_defer = int(max_defer)
        if not 0 <= max_defer <= 0x7FFFFFFF:
            raise SlideoError(1, "gate settle: max_defer %d outside 0 .. 2**31 - 1" % max_defer)
        self._check(getattr(lib(), self._SETS + "set_gate_settle")(self._h, C.c_float(similarity), max_defer))

    def gate_settle(self):
        """(similarity, max_defer); (0.0, 0) unless set (a Group: member 0's)."""
        s, d = C.c_float(), C.c_int32()
        rc = lib().slideo_matcher_gate_settle(self._mask_owner(), C.byref(s), C.byref(d))
        if rc != OK:
            raise SlideoError(rc, "gate_settle")
        return s.value, d.value

    # gate memory (include/slideo_amd.h "Gate memory"): under 'anchor', recall the verdict of an earlier matched frame
    def set_gate_memory(self, capacity):
        """capacity: 0 (off, the default) or 1 .. GATE_MEMORY_MAX: the last `capacity` matched frames are remembered, and a frame away
        from the anchor that is within changed_similarity of one of them is recalled (changed == 0, last_gate_refs() names the frame
        it stands behind).  Needs the gate reference 'anchor'; the matcher must be idle; resets the gate state.  A Group of more than
        one member refuses a memory that is on."""
        capacity = int(capacity)
        if not 0 <= capacity <= GATE_MEMORY_MAX:
            raise SlideoError(1, "gate memory: capacity %d outside 0 .. %d" % (capacity, GATE_MEMORY_MAX))
        self._check(getattr(lib(), self._SETS + "set_gate_memory")(self._h, capacity))

    def gate_memory(self):
        """The gate memory's capacity; 0 unless set (a Group: member 0's)."""
        c = C.c_int32()
        rc = lib().slideo_matcher_gate_memory(self._mask_owner(), C.byref(c))
        if rc != OK:
            raise SlideoError(rc, "gate_memory")
        return c.value

    def last_gate_refs(self):
        """int64 [n]: for every frame of the last synchronous gated call, or of the last collected gated ticket, the ordinal of the
        matched frame it stands behind (its own when it was matched), GATE_REF_RESET or GATE_REF_DEFERRED."""
        f = getattr(lib(), self._SETS + "last_gate_refs")
        n = C.c_int64()
        rc = f(self._h, None, 0, C.byref(n))
        if rc not in (OK, 7):                                    # (SLIDEO_ERR_CAPACITY: *n is the size to ask with)
            self._check(rc)
        out = np.empty(n.value, np.int64)
        self._check(f(self._h, _p(out), n.value, C.byref(n)))
        return out

    # YUV colour description (include/slideo_amd.h "YUV colour description"): how every *_yuv420 call reads its samples
    def set_yuv_description(self, matrix="bt601", range="limited", depth=8):
        """matrix: 'bt601' | 'bt709'; range: 'limited' | 'full'; depth: 8, '10_msb' (P010: 16-bit containers, value in the top
        10 bits) or '10_lsb' (yuv420p10le) — or the SLIDEO_YUV_* values.  The default (bt601, limited, 8) is cvtColor's reading.
        Under a 10-bit depth layouts count BYTES of 16-bit containers (yuv420_layout(..., bytes_per_sample=2)).  The matcher must
        be idle; ends the kept frames and resets the gate state."""
        self._check(getattr(lib(), self._SETS + "set_yuv_description")(
            self._h, _yuv_enum(YUV_MATRICES, matrix, "matrix"), _yuv_enum(YUV_RANGES, range, "range"), _yuv_enum(YUV_DEPTHS, depth, "depth")))

    def yuv_description(self):
        """(matrix, range, depth) as the SLIDEO_YUV_* values (a Group: member 0's)."""
        v = [C.c_int32() for _ in range(3)]
        rc = lib().slideo_matcher_yuv_description(self._mask_owner(), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]))
        if rc != OK:
            raise SlideoError(rc, "yuv_description")
        return v[0].value, v[1].value, v[2].value

    # YUV sampling (include/slideo_amd.h "YUV sampling"): where every *_yuv420 call finds its samples
    def set_yuv_sampling(self, sampling="420"):
        """'420' (the default) | '422' | '444' | '422_packed' — or the SLIDEO_YUV_SAMPLING_* value.  Every call that takes a layout
        then reads 4:2:2 / 4:4:4 planes (yuv_layout('nv16' ...)) or packed macropixels ('yuy2', 'uyvy' ...); the names keep their
        `420`.  The matcher must be idle; ends the kept frames and resets the gate state.  set_yuv_description leaves it alone."""
        if isinstance(sampling, str):
            if sampling.lower() not in YUV_SAMPLINGS:
                raise SlideoError(1, "yuv sampling: unknown %r (one of %s)" % (sampling, sorted(YUV_SAMPLINGS)))
            sampling = YUV_SAMPLINGS[sampling.lower()]
        self._check(getattr(lib(), self._SETS + "set_yuv_sampling")(self._h, int(sampling)))

    def yuv_sampling(self):
        """The SLIDEO_YUV_SAMPLING_* value (a Group: member 0's)."""
        v = C.c_int32()
        rc = lib().slideo_matcher_yuv_sampling(self._mask_owner(), C.byref(v))
        if rc != OK:
            raise SlideoError(rc, "yuv_sampling")
        return v.value

    # YUV chroma filter (include/slideo_amd.h "YUV chroma filter"): how a pixel's chroma is read from the samples
    def set_yuv_chroma(self, filt="nearest"):
        """'nearest' (the default) | 'left' (H.264 / HEVC / MPEG-2) | 'center' (JPEG, MPEG-1) | 'topleft' (BT.2020 / UHD) — or the
        SLIDEO_YUV_CHROMA_* value.  Every call that takes a layout then reads the chroma of 4:2:0 and 4:2:2 frames through the
        bilinear filter of that siting; 4:4:4 frames are untouched.  ValueError for an unknown name.  The matcher must be idle; ends
        the kept frames and resets the gate state.  set_yuv_description and set_yuv_sampling leave it alone."""
        self._check(getattr(lib(), self._SETS + "set_yuv_chroma")(self._h, yuv_chroma_value(filt)))

    def yuv_chroma(self):
        """The SLIDEO_YUV_CHROMA_* value (a Group: member 0's)."""
        v = C.c_int32()
        rc = lib().slideo_matcher_yuv_chroma(self._mask_owner(), C.byref(v))
        if rc != OK:
            raise SlideoError(rc, "yuv_chroma")
        return v.value

    # YUV transfer (include/slideo_amd.h "YUV transfer"): HLG and PQ BT.2020 frames to SDR
    def set_yuv_transfer(self, transfer="sdr", white_nits=0):
        """'sdr' (the default) | 'hlg' (ARIB STD-B67 / BT.2100) | 'pq' (SMPTE ST 2084) — or the SLIDEO_YUV_TRANSFER_* value; both
        with BT.2020 primaries and the BT.2020 non-constant-luminance matrix (the description's matrix is not consulted; its range
        and depth are).  white_nits: the display light that becomes SDR white — 0 means 203; else 1 .. 10000; 0 under 'sdr'.  Needs
        a 10-bit depth and nearest chroma (or 4:4:4).  ValueError for an unknown name.  The matcher must be idle; ends the kept
        frames and resets the gate state.  set_yuv_description, set_yuv_sampling and set_yuv_chroma leave it alone."""
        self._check(getattr(lib(), self._SETS + "set_yuv_transfer")(self._h, yuv_transfer_value(transfer), C.c_float(white_nits)))

    def yuv_transfer(self):
        """(SLIDEO_YUV_TRANSFER_* value, white_nits in force: 203.0 for a 0, 0.0 under SDR) (a Group: member 0's)."""
        t, n = C.c_int32(), C.c_float()
        rc = lib().slideo_matcher_yuv_transfer(self._mask_owner(), C.byref(t), C.byref(n))
        if rc != OK:
            raise SlideoError(rc, "yuv_transfer")
        return t.value, n.value

    # frame pixel format (include/slideo_amd.h "Frame pixel format"): how every *_bgr8 frame call reads its frames
    def set_pixel_format(self, fmt="bgr"):
        """'bgr' (the default) | 'rgb' | 'bgra' | 'rgba' | 'argb' | 'abgr' | 'planar_rgb' | 'planar_bgr' | 'planar_gbr' — or the
        SLIDEO_PIXEL_* value.  Every frame call of the BGR door then reads its frames under it (host arrays [n, h, w, 3],
        [n, h, w, 4] or [n, 3, h, w]); pages and single-image taps stay BGR.  The matcher must be idle; ends the kept frames and
        resets the gate state."""
        self._check(getattr(lib(), self._SETS + "set_pixel_format")(self._h, pixel_format_value(fmt)))

    def pixel_format(self):
        """The SLIDEO_PIXEL_* value (a Group: member 0's)."""
        if not hasattr(lib(), "slideo_matcher_pixel_format"):       # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            return 0
        v = C.c_int32()
        rc = lib().slideo_matcher_pixel_format(self._mask_owner(), C.byref(v))
        if rc != OK:
            raise SlideoError(rc, "pixel_format")
        return v.value

    # frame levels (include/slideo_amd.h "Frame levels"): a per-channel tone table, the last step in front of the unit's image
    def set_frame_levels(self, lut=None):
        """lut: uint8 [3, 256] (B, G, R), or None (= the identity) for off.  Every frame call then analyses lut[c][image]; pages and
        single-image taps are untouched.  The matcher must be idle and its levels histogram closed; ends the kept frames and resets
        the gate state."""
        if lut is not None:
            lut = _levels_table(lut)
        self._check(getattr(lib(), self._SETS + "set_frame_levels")(self._h, _p(lut) if lut is not None else None))

    def frame_levels(self):
        """The table uint8 [3, 256] in force, or None when off (a Group: member 0's)."""
        if not hasattr(lib(), "slideo_matcher_frame_levels"):       # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            return None
        out, on = np.empty((3, 256), np.uint8), C.c_int32()
        rc = lib().slideo_matcher_frame_levels(self._mask_owner(), _p(out), C.byref(on))
        if rc != OK:
            raise SlideoError(rc, "frame_levels")
        return out if on.value else None

    # frame shading (include/slideo_amd.h "Frame shading"): a bilinear Q8.8 gain field on the unit's image, in front of the levels
    def set_frame_shading(self, aw=0, ah=0, cell=0, gains=None):
        """gains: uint16 [gh + 1, gw + 1] Q8.8 nodes over the aw x ah analysed image at `cell` (16, 32, 64), or None (= all 256) for
        off.  Every frame call then analyses min(255, (image * G + 128) >> 8); pages and single-image taps are untouched.  The
        matcher must be idle; ends the kept frames and the match sessions and resets the gate state."""
        if gains is not None:
            aw, ah, cell, gains = _shading_field(aw, ah, cell, gains)
        self._check(getattr(lib(), self._SETS + "set_frame_shading")(self._h, int(aw), int(ah), int(cell), _p(gains) if gains is not None else None))

    def frame_shading(self):
        """(aw, ah, cell, gains uint16 [gh + 1, gw + 1]) in force, or None when off (a Group: member 0's)."""
        if not hasattr(lib(), "slideo_matcher_frame_shading"):      # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            return None
        aw, ah, cell, on = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        rc = lib().slideo_matcher_frame_shading(self._mask_owner(), None, C.c_int64(0), C.byref(aw), C.byref(ah), C.byref(cell), C.byref(on))
        if rc != OK:
            raise SlideoError(rc, "frame_shading")
        if not on.value:
            return None
        gw, gh = -(-aw.value // cell.value), -(-ah.value // cell.value)
        out = np.empty((gh + 1, gw + 1), np.uint16)
        rc = lib().slideo_matcher_frame_shading(self._mask_owner(), _p(out), C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(cell), C.byref(on))
        if rc != OK:
            raise SlideoError(rc, "frame_shading")
        return aw.value, ah.value, cell.value, out

    def _mask_owner(self):
        """The matcher handle the mask's getters read (a group's members agree: member 0)."""
        return self._h if self._SETS == "slideo_matcher_" else C.c_void_p(lib().slideo_group_member(self._h, 0))

    @property
    def frame_mask_scope(self):
        scope = C.c_uint32()
        rc = lib().slideo_matcher_frame_mask_scope(self._mask_owner(), C.byref(scope))
        if rc != OK:
            raise SlideoError(rc, "frame_mask_scope")
        return scope.value

    def frame_mask_small(self):
        """The gate's validity map under MASK_GATE: (bool [sh, sw], n_valid)."""
        h = self._mask_owner()
        sw, sh, nv = C.c_int32(), C.c_int32(), C.c_int64()

        def check(rc):
            if rc != OK:
                raise SlideoError(rc, lib().slideo_last_error(h).decode())
        check(lib().slideo_frame_mask_small(h, None, C.c_int64(0), C.byref(sw), C.byref(sh), C.byref(nv)))
        out = np.empty((sh.value, sw.value), np.uint8)
        check(lib().slideo_frame_mask_small(h, _p(out), C.c_int64(out.size), C.byref(sw), C.byref(sh), C.byref(nv)))
        return out == 255, int(nv.value)

    # frame region (include/slideo_amd.h "Frame region"): frames of the region's source size stand for their rectified image
    def set_frame_region(self, src_w, src_h, M, out_w, out_h):
        """M: a 3x3 map (9 floats) from the rectified out_w x out_h image into src_w x src_h frames, or a quad — 4 (x, y) source
        corners: top-left, top-right, bottom-right, bottom-left (frame_region_from_quad).  The matcher must be idle."""
        M = np.asarray(M, np.float64)
        if M.size == 8:
            M = frame_region_from_quad(M, out_w, out_h)
        if M.size != 9:
            raise SlideoError(1, "set_frame_region: expected a 3x3 map or a 4x2 quad")
        M = np.ascontiguousarray(M.reshape(9))
        self._check(getattr(lib(), self._SETS + "set_frame_region")(self._h, int(src_w), int(src_h), _p(M), int(out_w), int(out_h)))

    def clear_frame_region(self):
        self._check(getattr(lib(), self._SETS + "set_frame_region")(self._h, 0, 0, None, 0, 0))

    @property
    def frame_region(self):
        """(src_w, src_h, M [3, 3], out_w, out_h), or None."""
        if not hasattr(lib(), "slideo_matcher_frame_region"):       # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            return None
        h = self._mask_owner()
        v = [C.c_int32() for _ in range(5)]
        M = np.zeros(9, np.float64)
        rc = lib().slideo_matcher_frame_region(h, C.byref(v[0]), C.byref(v[1]), _p(M), C.byref(v[2]), C.byref(v[3]), C.byref(v[4]))
        if rc != OK:
            raise SlideoError(rc, "frame_region")
        return (v[0].value, v[1].value, M.reshape(3, 3), v[2].value, v[3].value) if v[4].value else None

    def rectify(self, bgr):
        """The rectified image of one host image under the region (the rectify tap; a Group: member 0's)."""
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        return self.rectify_pitched(bgr, w, h, w * 3)

    def rectify_pitched(self, buf, w, h, stride):
        """The same for an image of w x h in `buf` with rows `stride` bytes apart."""
        buf = np.ascontiguousarray(buf, np.uint8)
        reg = self.frame_region
        ow, oh = (reg[3], reg[4]) if reg else (0, 0)
        out = np.empty((oh, ow, 3), np.uint8)
        hd = self._mask_owner()
        rc = lib().slideo_rectify_bgr8(hd, _p(buf), int(w), int(h), int(stride), _p(out), C.c_int64(out.size))
        if rc != OK:
            raise SlideoError(rc, lib().slideo_last_error(hd).decode())
        return out

    frame_region_from_quad = staticmethod(lambda quad, out_w, out_h: frame_region_from_quad(quad, out_w, out_h))

    # frame lens (include/slideo_amd.h "Frame lens"): frames of the lens's source size are undistorted in the rectify's launch
    def set_frame_lens(self, src_w, src_h, cx=None, cy=None, f=None, k1=0.0, k2=0.0):
        """The radial lens c + (p - c) (1 + k1 r2 + k2 r2^2), r2 = |p - c|^2 / f^2.  cx, cy None: the image centre ((src_w - 1) / 2,
        (src_h - 1) / 2); f None: half the source diagonal, so that k1 is the relative displacement at the corner.  k1 == k2 == 0:
        off.  The matcher must be idle."""
        cx, cy, f = frame_lens_defaults(src_w, src_h, cx, cy, f)
        self._check(getattr(lib(), self._SETS + "set_frame_lens")(self._h, int(src_w), int(src_h), float(cx), float(cy), float(f), float(k1), float(k2)))

    def clear_frame_lens(self):
        self._check(getattr(lib(), self._SETS + "set_frame_lens")(self._h, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0))

    @property
    def frame_lens(self):
        """(src_w, src_h, cx, cy, f, k1, k2), or None."""
        if not hasattr(lib(), "slideo_matcher_frame_lens"):         # (SLIDEO_LIB_PATH may name an older build: tools/ab_libs.sh)
            return None
        h = self._mask_owner()
        s = [C.c_int32(), C.c_int32()]
        d = [C.c_double() for _ in range(5)]
        on = C.c_int32()
        rc = lib().slideo_matcher_frame_lens(h, C.byref(s[0]), C.byref(s[1]), *[C.byref(x) for x in d], C.byref(on))
        if rc != OK:
            raise SlideoError(rc, "frame_lens")
        return (s[0].value, s[1].value) + tuple(x.value for x in d) if on.value else None

    def undistort(self, bgr):
        """The analysed image of one host image under the lens, and the region if one is set (the tap; a Group: member 0's)."""
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        return self.undistort_pitched(bgr, w, h, w * 3)

    def undistort_pitched(self, buf, w, h, stride):
        """The same for an image of w x h in `buf` with rows `stride` bytes apart."""
        buf = np.ascontiguousarray(buf, np.uint8)
        lens, reg = self.frame_lens, self.frame_region
        ow, oh = (reg[3], reg[4]) if reg else (lens[0], lens[1]) if lens else (0, 0)
        out = np.empty((oh, ow, 3), np.uint8)
        hd = self._mask_owner()
        rc = lib().slideo_undistort_bgr8(hd, _p(buf), int(w), int(h), int(stride), _p(out), C.c_int64(out.size))
        if rc != OK:
            raise SlideoError(rc, lib().slideo_last_error(hd).decode())
        return out

    def _unit_size(self, w, h):
        """The size of the image the pipeline reads for a w x h frame."""
        reg = self.frame_region
        if reg is not None:
            return reg[3], reg[4]
        lens = self.frame_lens
        if lens is not None:
            return lens[0], lens[1]
        mw, mh = self.working_size
        return working_size(w, h, mw, mh) if mw > 0 else (w, h)

    # page sets (include/slideo_amd.h "page sets"): frame calls made while a set is selected search its pages only.  The argument
    # rules the library checks are checked here first, so that a bad call fails the same way before any device is involved.
    _SETS = None        # symbol prefix of the set calls: "slideo_matcher_" / "slideo_group_"

    def create_page_set(self, pages):
        """pages: distinct deck page indices (any order) -> the set's id (>= 1)."""
        arr = _page_set_pages(pages)
        out = C.c_int32()
        self._check(getattr(lib(), self._SETS + "create_page_set")(self._h, len(arr), _p(arr), C.byref(out)))
        return int(out.value)

    def use_page_set(self, set_id):
        """Frame calls from now on search `set_id` (0 = the whole deck); units already in flight keep theirs."""
        self._check(getattr(lib(), self._SETS + "use_page_set")(self._h, _page_set_id(set_id, 0)))

    def release_page_set(self, set_id):
        self._check(getattr(lib(), self._SETS + "release_page_set")(self._h, _page_set_id(set_id, 1)))


def _page_set_pages(pages):
    """A page set's index list as int32, with the library's argument rules (SLIDEO_ERR_INVALID_ARG) applied on the host."""
    arr = np.asarray(list(pages) if not isinstance(pages, np.ndarray) else pages).reshape(-1)
    if arr.size < 1:
        raise SlideoError(1, "a page set needs at least one page")
    if arr.dtype.kind not in "iu":
        raise SlideoError(1, "page indices must be integers (got %s)" % arr.dtype)
    if (arr < 0).any() or (arr > np.iinfo(np.int32).max).any():
        raise SlideoError(1, "page index %d out of range" % int(arr[(arr < 0) | (arr > np.iinfo(np.int32).max)][0]))
    if len(np.unique(arr)) != arr.size:
        raise SlideoError(1, "a page is listed twice")
    return np.ascontiguousarray(arr, np.int32)


def _page_set_id(set_id, lowest):
    if isinstance(set_id, bool) or not isinstance(set_id, (int, np.integer)) or not lowest <= int(set_id) <= np.iinfo(np.int32).max:
        raise SlideoError(1, "page set id %r is not one the library hands out" % (set_id,))
    return int(set_id)


class Matcher(_FrameCalls):
    """Owns one slideo_matcher handle (page database + workspace on one GPU)."""
    _PREFIX = "slideo_"
    _SETS = "slideo_matcher_"

    def __init__(self, cfg=None, device=0):
        self.cfg = cfg if cfg is not None else default_config()
        self._h = C.c_void_p()
        self._cb = None
        rc = lib().slideo_matcher_create(C.byref(self.cfg), int(device), C.byref(self._h))
        if rc != OK:
            raise SlideoError(rc, lib().slideo_last_error(None).decode())

    def _check(self, rc):
        if rc != OK:
            raise SlideoError(rc, lib().slideo_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().slideo_matcher_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_progress(self, fn):
        """fn(done, total, msg) or None."""
        if fn is None:
            self._cb = None
            self._check(lib().slideo_matcher_set_progress(self._h, None, None))
            return
        self._cb = PROGRESS_FN(lambda user, d, t, msg: fn(int(d), int(t), (msg or b"").decode()))
        self._check(lib().slideo_matcher_set_progress(self._h, self._cb, None))

    # ---- pages -------------------------------------------------------------------
    def add_pages(self, pages):
        pages = [_img3(p) for p in pages]
        n = len(pages)
        ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in pages])
        w = (C.c_int32 * n)(*[p.shape[1] for p in pages])
        h = (C.c_int32 * n)(*[p.shape[0] for p in pages])
        s = (C.c_int32 * n)(*[p.shape[1] * 3 for p in pages])
        self._check(lib().slideo_matcher_add_pages_bgr8(self._h, n, ptrs, w, h, s))

    def page_set_info(self, set_id):
        """-> {n_pages, rows, unique_rows, bytes} of set `set_id` (0: the whole deck)."""
        n, rows, urows, nbytes = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(lib().slideo_matcher_page_set_info(self._h, _page_set_id(set_id, 0), C.byref(n), C.byref(rows), C.byref(urows),
                                                       C.byref(nbytes)))
        return {"n_pages": n.value, "rows": rows.value, "unique_rows": urows.value, "bytes": nbytes.value}

    def page_small(self, page):
        """Small image of a page (to_small_image), as slideo_matcher_get_page_small returns it."""
        sw = C.c_int32(); sh = C.c_int32()
        rc = lib().slideo_matcher_get_page_small(self._h, page, None, C.c_int64(1 << 40), C.byref(sw), C.byref(sh))
        self._check(rc)
        out = np.empty((sh.value, sw.value, 3), np.uint8)
        self._check(lib().slideo_matcher_get_page_small(self._h, page, _p(out), C.c_int64(out.size), C.byref(sw), C.byref(sh)))
        return out

    def add_page_features(self, width, height, kp, desc, small):
        """A page analysed elsewhere (another rank's share of the deck, a cache): slideo_matcher_add_page_features."""
        kp = np.ascontiguousarray(kp, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        small = np.ascontiguousarray(small, np.uint8)
        assert len(kp) == len(desc) and small.ndim == 3 and small.shape[2] == 3
        self._check(lib().slideo_matcher_add_page_features(self._h, int(width), int(height), len(kp), _p(kp), _p(desc), _p(small),
                                                           small.shape[1], small.shape[0]))

    def finalize(self):
        self._check(lib().slideo_matcher_finalize_pages(self._h))

    @property
    def page_count(self):
        return int(lib().slideo_matcher_page_count(self._h))

    @property
    def descriptor_count(self):
        return int(lib().slideo_matcher_descriptor_count(self._h))

    @property
    def working_size(self):
        mw, mh = C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_get_working_size(self._h, C.byref(mw), C.byref(mh)))
        return mw.value, mh.value

    @property
    def unique_descriptor_count(self):
        """Distinct rows among the train descriptors: what the k-NN stage actually searches (results are those of all rows)."""
        return int(lib().slideo_matcher_unique_descriptor_count(self._h))

    def use_sift(self, sift_cfg, ratio=0.0):
        """SIFT features + the squared-L2 search in front of the path's own vote / RANSAC / re-projection stages (north-star /
        configs[2] as a complete matcher).  ratio in (0, 1]: Lowe's ratio test on the two nearest rows; ratio 0: the path's
        tolerance vote on the knn_k nearest rows.  Before the first page."""
        self._check(lib().slideo_matcher_use_sift(self._h, C.byref(sift_cfg), C.c_float(ratio)))
        self._sift = True

    def page_features(self, page):
        n = C.c_int32()
        rc = lib().slideo_matcher_get_page_features(self._h, page, None, None, 0, C.byref(n))
        if rc not in (OK, 7):
            self._check(rc)
        kp = np.zeros(n.value, KEYPOINT_DTYPE)
        desc = np.zeros((n.value, 128 if getattr(self, "_sift", False) else 32), np.uint8)
        self._check(lib().slideo_matcher_get_page_features(self._h, page, _p(kp), _p(desc), n.value, C.byref(n)))
        return kp, desc

    # ---- frames (the host calls: _FrameCalls) --------------------------------------------
    def match_frames_dev(self, dev_ptr, n, w, h, stride=None, frame_stride=None, stream=0):
        """Frames already resident in HBM (raw device pointer)."""
        stride, frame_stride = self._pix_strides(w, h, stride, frame_stride)
        out = np.zeros(n, VERDICT_DTYPE)
        self._check(lib().slideo_match_frames_bgr8_dev(self._h, n, C.c_void_p(dev_ptr), w, h, stride,
                                                       C.c_int64(frame_stride), _p(out),
                                                       C.c_void_p(stream)))
        return out

    # ---- frame lists: the forms a single matcher has beyond _FrameCalls' ----
    def submit_list(self, fl, stream=0):
        """Streaming form of a DEVICE list: a ticket for collect.  The record is copied at the call; the frames stay valid until collect."""
        t = C.c_int64()
        self._check(lib().slideo_match_frames_submit_list(self._h, fl.ref(), C.c_void_p(stream or None), C.byref(t)))
        return (t.value, fl.n)

    def submit_changed_list(self, fl, stream=0):
        t = C.c_int64()
        self._check(lib().slideo_match_changed_frames_submit_list(self._h, fl.ref(), C.c_void_p(stream or None), C.byref(t)))
        return (t.value, fl.n)

    def observe_frames_list(self, fl, stream=0):
        self._check(lib().slideo_matcher_observe_frames_list(self._h, fl.ref(), C.c_void_p(stream or None)))

    def gate_reset_from_frame_list(self, fl, stream=0):
        """The gate state from a list of one frame."""
        self._check(lib().slideo_matcher_gate_reset_from_frame_list(self._h, fl.ref(), C.c_void_p(stream or None)))

    def frame_list_to_bgr8(self, fl):
        """Tap: the BGR image at source size of every frame of the list -> uint8 [n, h, w, 3]."""
        out = np.zeros((fl.n, fl.height, fl.width, 3), np.uint8)
        self._check(lib().slideo_frame_list_to_bgr8(self._h, fl.ref(), _p(out), C.c_int64(out.size)))
        return out

    def rng_stream_len(self):
        """The length of the pre-drawn RNG stream now (it grows when a unit outran it and was run again)."""
        n = C.c_int64()
        self._check(lib().slideo_matcher_rng_stream_len(self._h, C.byref(n)))
        return n.value

    def max_in_flight(self):
        return int(lib().slideo_matcher_max_in_flight(self._h))

    def submit_dev(self, dev_ptr, n, w, h, stride=None, frame_stride=None, stream=0):
        """Streaming form: returns a ticket; at most max_in_flight() units in flight; collect in order."""
        stride, frame_stride = self._pix_strides(w, h, stride, frame_stride)
        t = C.c_int64()
        self._check(lib().slideo_match_frames_submit_dev(self._h, n, C.c_void_p(dev_ptr), w, h, stride,
                                                         C.c_int64(frame_stride), C.c_void_p(stream), C.byref(t)))
        return (t.value, n)

    def collect(self, ticket, dev_out=0):
        """dev_out: optional device pointer that also receives the n verdict records (16 bytes each)."""
        t, n = ticket
        out = np.zeros(n, VERDICT_DTYPE)
        self._check(lib().slideo_match_frames_collect_dev(self._h, C.c_int64(t), _p(out), C.c_void_p(dev_out or None)))
        return out

    # ---- changed-frame gate (include/slideo_amd.h "Changed-frame gate") ------------------------
    # Gated calls return (changed [n] bool, similarity [n] f32, verdicts [n]); an unchanged frame's verdict is (-1, 0, 0, 0).
    def gate_reset_from_frame(self, frame):
        """The gate state from one host frame ([h, w, 3] BGR, or the shape of the pixel format in force): what
        gate_reset(changed_mask([frame])'s last small image) leaves."""
        frame, _, w, h, st, _ = self._pix_frames(np.asarray(frame)[None], "gate_reset_from_frame")
        self._check(lib().slideo_matcher_gate_reset_from_frame_bgr8(self._h, _p(frame), w, h, st))

    def gate_reset_from_frame_yuv420(self, frame, w, h, layout="nv12"):
        frames, layout, _ = _yuv_frames(np.asarray(frame).reshape(-1), w, h, layout)
        self._check(lib().slideo_matcher_gate_reset_from_frame_yuv420(self._h, _p(frames), w, h, C.byref(layout)))

    def gate_reset_from_frame_dev(self, dev_ptr, w, h, stride=None, stream=0):
        stride, _ = self._pix_strides(w, h, stride, None)
        self._check(lib().slideo_matcher_gate_reset_from_frame_bgr8_dev(self._h, C.c_void_p(dev_ptr), w, h, stride, C.c_void_p(stream)))

    def gate_reset_from_frame_yuv420_dev(self, dev_ptr, w, h, layout, stream=0):
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        self._check(lib().slideo_matcher_gate_reset_from_frame_yuv420_dev(self._h, C.c_void_p(dev_ptr), w, h, C.byref(layout), C.c_void_p(stream)))

    def match_changed_frames_dev(self, dev_ptr, n, w, h, stride=None, frame_stride=None, stream=0):
        stride, frame_stride = self._pix_strides(w, h, stride, frame_stride)
        ch, sim, out = self._gated_out(n)
        self._check(lib().slideo_match_changed_frames_bgr8_dev(self._h, n, C.c_void_p(dev_ptr), w, h, stride, C.c_int64(frame_stride),
                                                               _p(ch), _p(sim), _p(out), C.c_void_p(stream)))
        return ch.astype(bool), sim, out

    def match_changed_frames_yuv420_dev(self, dev_ptr, n, w, h, layout, frame_stride, stream=0):
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        ch, sim, out = self._gated_out(n)
        self._check(lib().slideo_match_changed_frames_yuv420_dev(self._h, n, C.c_void_p(dev_ptr), w, h, C.byref(layout),
                                                                 C.c_int64(frame_stride), _p(ch), _p(sim), _p(out), C.c_void_p(stream)))
        return ch.astype(bool), sim, out

    def submit_changed_dev(self, dev_ptr, n, w, h, stride=None, frame_stride=None, stream=0):
        """A gated unit (streaming form): a ticket for collect_changed; tickets of gated and plain units share one order."""
        stride, frame_stride = self._pix_strides(w, h, stride, frame_stride)
        t = C.c_int64()
        self._check(lib().slideo_match_changed_frames_submit_dev(self._h, n, C.c_void_p(dev_ptr), w, h, stride, C.c_int64(frame_stride),
                                                                 C.c_void_p(stream), C.byref(t)))
        return (t.value, n)

    def submit_changed_yuv420_dev(self, dev_ptr, n, w, h, layout, frame_stride, stream=0):
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        t = C.c_int64()
        self._check(lib().slideo_match_changed_frames_submit_yuv420_dev(self._h, n, C.c_void_p(dev_ptr), w, h, C.byref(layout),
                                                                        C.c_int64(frame_stride), C.c_void_p(stream), C.byref(t)))
        return (t.value, n)

    def collect_changed(self, ticket):
        t, n = ticket
        ch, sim, out = self._gated_out(n)
        self._check(lib().slideo_match_changed_frames_collect(self._h, C.c_int64(t), _p(ch), _p(sim), _p(out)))
        return ch.astype(bool), sim, out

    # ---- frame activity map (include/slideo_amd.h "Frame activity map") ------------------------
    def activity_begin(self, delta):
        """An empty accumulator: a pixel moved between consecutive observed images iff its BGR sum of absolute differences > delta."""
        self._check(lib().slideo_matcher_activity_begin(self._h, int(delta)))

    def activity_end(self):
        self._check(lib().slideo_matcher_activity_end(self._h))

    def observe_frames(self, frames):
        """frames: uint8 [n, h, w, 3] in host memory (the array shape of the pixel format in force), continuing the accumulator."""
        frames, n, w, h, st, fs = self._pix_frames(frames, "observe_frames")
        self._check(lib().slideo_matcher_observe_frames_bgr8(self._h, n, _p(frames), w, h, st, C.c_int64(fs)))

    def observe_frames_yuv420(self, frames, w, h, layout="nv12"):
        frames, layout, fs = _yuv_frames(frames, w, h, layout)
        self._check(lib().slideo_matcher_observe_frames_yuv420(self._h, frames.shape[0], _p(frames), w, h, C.byref(layout), C.c_int64(fs)))

    def observe_frames_dev(self, dev_ptr, n, w, h, stride=None, frame_stride=None, stream=0):
        stride, frame_stride = self._pix_strides(w, h, stride, frame_stride)
        self._check(lib().slideo_matcher_observe_frames_bgr8_dev(self._h, n, C.c_void_p(dev_ptr), w, h, stride, C.c_int64(frame_stride),
                                                                 C.c_void_p(stream)))

    def observe_frames_yuv420_dev(self, dev_ptr, n, w, h, layout, frame_stride, stream=0):
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        self._check(lib().slideo_matcher_observe_frames_yuv420_dev(self._h, n, C.c_void_p(dev_ptr), w, h, C.byref(layout),
                                                                   C.c_int64(frame_stride), C.c_void_p(stream)))

    def activity_info(self):
        """-> {aw, ah, pairs, delta} (aw == 0 before the first observed frame)."""
        aw, ah, pairs, delta = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_activity_info(self._h, C.byref(aw), C.byref(ah), C.byref(pairs), C.byref(delta)))
        return {"aw": aw.value, "ah": ah.value, "pairs": pairs.value, "delta": delta.value}

    def activity_counts(self):
        """-> (counts uint32 [ah, aw], pairs)"""
        aw, ah, pairs = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_activity_counts(self._h, None, C.c_int64(0), C.byref(aw), C.byref(ah), C.byref(pairs)))
        out = np.empty((ah.value, aw.value), np.uint32)
        self._check(lib().slideo_matcher_activity_counts(self._h, _p(out), C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(pairs)))
        return out, pairs.value

    def activity_mask(self, max_share, grow):
        """max_share: a float in [0, 1], rounded to parts per million -> (mask uint8 [ah, aw] of 0 / 255, n_active, n_masked)"""
        i = self.activity_info()
        out = np.empty((i["ah"], i["aw"]), np.uint8)
        aw, ah, na, nm = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._check(lib().slideo_matcher_activity_mask(self._h, int(round(float(max_share) * 1000000)), int(grow), _p(out), C.c_int64(out.size),
                                                       C.byref(aw), C.byref(ah), C.byref(na), C.byref(nm)))
        return out, na.value, nm.value

    # ---- frame content box (include/slideo_amd.h "Frame content box") --------------------------
    def content_begin(self, level):
        """An empty content accumulator: a pixel of an observed image is lit iff max(B, G, R) > level.  observe_frames* feed it."""
        self._check(lib().slideo_matcher_content_begin(self._h, int(level)))

    def content_end(self):
        self._check(lib().slideo_matcher_content_end(self._h))

    def content_info(self):
        """-> {aw, ah, frames, level} (aw == 0 before the first observed frame)."""
        aw, ah, frames, level = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_content_info(self._h, C.byref(aw), C.byref(ah), C.byref(frames), C.byref(level)))
        return {"aw": aw.value, "ah": ah.value, "frames": frames.value, "level": level.value}

    def content_counts(self):
        """-> (lit uint32 [ah, aw], frames)"""
        aw, ah, frames = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_content_counts(self._h, None, C.c_int64(0), C.byref(aw), C.byref(ah), C.byref(frames)))
        out = np.empty((ah.value, aw.value), np.uint32)
        self._check(lib().slideo_matcher_content_counts(self._h, _p(out), C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(frames)))
        return out, frames.value

    def content_box(self, min_share, min_fill):
        """min_share, min_fill: floats in [0, 1], rounded to parts per million -> ((x0, y0, x1, y1), n_content, row_fill uint32 [ah],
        col_fill uint32 [aw])"""
        i = self.content_info()
        fill = np.empty(i["ah"] + i["aw"], np.uint32)
        box, nc = (C.c_int32 * 4)(), C.c_int64()
        self._check(lib().slideo_matcher_content_box(self._h, int(round(float(min_share) * 1000000)), int(round(float(min_fill) * 1000000)), box,
                                                     C.byref(nc), _p(fill), C.c_int64(fill.size)))
        return tuple(box), nc.value, fill[:i["ah"]].copy(), fill[i["ah"]:].copy()

    # ---- YUV 4:2:0 frames (include/slideo_amd.h "YUV 4:2:0 frames") ---------------------------
    def match_frames_yuv420_dev(self, dev_ptr, n, w, h, layout, frame_stride, stream=0):
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        out = np.zeros(n, VERDICT_DTYPE)
        self._check(lib().slideo_match_frames_yuv420_dev(self._h, n, C.c_void_p(dev_ptr), w, h, C.byref(layout), C.c_int64(frame_stride),
                                                         _p(out), C.c_void_p(stream)))
        return out

    def submit_yuv420_dev(self, dev_ptr, n, w, h, layout, frame_stride, stream=0):
        """As submit_dev; collect() collects it."""
        if isinstance(layout, str):
            layout = yuv_layout(layout, w, h)[0]
        t = C.c_int64()
        self._check(lib().slideo_match_frames_submit_yuv420_dev(self._h, n, C.c_void_p(dev_ptr), w, h, C.byref(layout),
                                                                C.c_int64(frame_stride), C.c_void_p(stream), C.byref(t)))
        return (t.value, n)

    # ---- frame levels: the tap and the learner (include/slideo_amd.h "Frame levels") ----------
    def levels_bgr(self, image, stride=None):
        """One host BGR image [h, w, 3] under the table in force (the tap; off: the image itself).  With `stride`: a (flat buffer, w,
        h) triple whose rows lie `stride` bytes apart (height * stride bytes are read)."""
        if stride is None:
            image = _img3(image)
            h, w, _ = image.shape
            stride = w * 3
        else:
            image, w, h = image
            image = np.ascontiguousarray(image, np.uint8)
            if image.size < h * int(stride):
                raise ValueError("levels_bgr: the buffer holds %d bytes, height * stride is %d" % (image.size, h * int(stride)))
        out = np.empty((h, w, 3), np.uint8)
        self._check(lib().slideo_levels_bgr8(self._h, _p(image), w, h, int(stride), _p(out), C.c_int64(out.size)))
        return out

    def shading_bgr(self, image, stride=None):
        """One host BGR image [h, w, 3] of the field's size through the shading step as a frame's unit image goes: the field and, with
        a levels table set, the table in the same pass (the tap; no field: the image itself).  `stride`: as levels_bgr."""
        if stride is None:
            image = _img3(image)
            h, w, _ = image.shape
            stride = w * 3
        else:
            image, w, h = image
            image = np.ascontiguousarray(image, np.uint8)
            if image.size < h * int(stride):
                raise ValueError("shading_bgr: the buffer holds %d bytes, height * stride is %d" % (image.size, h * int(stride)))
        out = np.empty((h, w, 3), np.uint8)
        self._check(lib().slideo_shading_bgr8(self._h, _p(image), w, h, int(stride), _p(out), C.c_int64(out.size)))
        return out

    def levels_begin(self):
        """An empty levels histogram; observe_frames* feed it.  Refused while a table is set."""
        self._check(lib().slideo_matcher_levels_begin(self._h))

    def levels_end(self):
        self._check(lib().slideo_matcher_levels_end(self._h))

    def levels_info(self):
        """-> {frames, pixels}"""
        fr, px = C.c_int64(), C.c_int64()
        self._check(lib().slideo_matcher_levels_info(self._h, C.byref(fr), C.byref(px)))
        return {"frames": fr.value, "pixels": px.value}

    def levels_histogram(self):
        """-> uint64 [3, 256] (B, G, R): the samples of every value of the observed images"""
        out = np.empty((3, 256), np.uint64)
        self._check(lib().slideo_matcher_levels_histogram(self._h, _p(out)))
        return out

    def levels_points(self, low, high):
        """low, high: the shares cut at either end, floats in [0, 1], rounded to parts per million -> (lo [3], hi [3]) as lists"""
        for name, v in (("low", low), ("high", high)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError("levels_points: %s = %r outside [0, 1]" % (name, v))
        lo, hi = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._check(lib().slideo_matcher_levels_points(self._h, int(round(float(low) * 1000000)), int(round(float(high) * 1000000)), lo, hi))
        return list(lo), list(hi)

    def pixels_to_bgr(self, frame, stride=None):
        """The BGR image (h, w, 3) one host frame stands for under the pixel format in force (the conversion tap).  frame: the
        format's array shape ([h, w, 3], [h, w, 4] or [3, h, w]); or, with `stride`, a (flat buffer, w, h) triple whose rows lie
        `stride` bytes apart."""
        if stride is None:
            frame, _, w, h, stride, _ = self._pix_frames(np.asarray(frame)[None], "pixels_to_bgr")
        else:
            frame, w, h = frame
            frame = np.ascontiguousarray(frame, np.uint8)
        out = np.empty((h, w, 3), np.uint8)
        self._check(lib().slideo_pixels_to_bgr8(self._h, _p(frame), w, h, int(stride), _p(out), C.c_int64(out.size)))
        return out

    def yuv420_to_bgr(self, frame, w, h, layout="nv12"):
        """The BGR image (h, w, 3) the library makes of one 4:2:0 frame (the conversion tap)."""
        frame, layout, _ = _yuv_frames(frame, w, h, layout)
        out = np.empty((h, w, 3), np.uint8)
        self._check(lib().slideo_yuv420_to_bgr8(self._h, _p(frame), w, h, C.byref(layout), _p(out), C.c_int64(out.size)))
        return out

    # ---- SIFT (north-star extension, csrc/sift.hip.h) ---------------------------------------
    def sift(self, bgr, scfg=None, cap=20000):
        """cv::SIFT::detectAndCompute on one host image: (keypoints, descriptors u8 [n, 128])."""
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        scfg = scfg or sift_config()
        kp = np.zeros(cap, KEYPOINT_DTYPE); desc = np.zeros((cap, 128), np.uint8)
        n = C.c_int32()
        rc = lib().slideo_sift_bgr8(self._h, C.byref(scfg), _p(bgr), w, h, w * 3, _p(kp), _p(desc), cap, C.byref(n))
        if rc == 7 and n.value > cap:
            return self.sift(bgr, scfg, cap=n.value)
        self._check(rc)
        return kp[: n.value].copy(), desc[: n.value].copy()

    def sift_layer(self, bgr, octave, layer, dog=False, scfg=None):
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        scfg = scfg or sift_config()
        out = np.empty(4 * h * w, np.float32)
        lw = C.c_int32(); lh = C.c_int32()
        self._check(lib().slideo_sift_layer_bgr8(self._h, C.byref(scfg), _p(bgr), w, h, w * 3, octave, layer, int(dog), _p(out),
                                                 C.c_int64(out.size), C.byref(lw), C.byref(lh)))
        return out[: lw.value * lh.value].reshape(lh.value, lw.value).copy()

    def sift_frames_dev(self, frames_ptr, n, w, h, kp_ptr, desc_ptr, capacity_total, scfg=None):
        """SIFT of n device frames into device arrays; returns (qofs [n + 1] host, kernel ms)."""
        scfg = scfg or sift_config()
        qofs = np.zeros(n + 1, np.uint32)
        ms = C.c_float()
        self._check(lib().slideo_sift_frames_dev(self._h, C.byref(scfg), n, C.c_void_p(frames_ptr), w, h, w * 3, C.c_int64(w * h * 3),
                                                 C.c_int64(capacity_total), C.c_void_p(kp_ptr), C.c_void_p(desc_ptr), _p(qofs), C.byref(ms)))
        return qofs, float(ms.value)

    def set_knn_engine(self, engine):
        """'mfma' (default: FP4 matrix cores, wave shape chosen per launch), 'mfma4' / 'mfma2' (the two shapes forced:
        2 waves/SIMD x 4 query tiles, 4 waves/SIMD x 2 query tiles) or 'valu' (integer popcount); identical results."""
        self._check(lib().slideo_matcher_set_knn_engine(self._h, {"mfma": 0, "valu": 1, "mfma4": 2, "mfma2": 3}[engine]))

    def set_knn_exact_lists(self, on=True):
        """Keep full exact k-NN lists in the matcher (default: only what the 5 % vote can use); same results."""
        self._check(lib().slideo_matcher_set_knn_exact_lists(self._h, int(bool(on))))

    # ---- measurement ------------------------------------------------------------------
    def set_profiling(self, enable=True):
        self._check(lib().slideo_matcher_set_profiling(self._h, int(bool(enable))))

    def read_profile(self):
        """-> dict(stage -> (ms, intervals)), knn_pairs; clears the accumulators."""
        ms = (C.c_double * 4)(); n = (C.c_int64 * 4)(); pairs = C.c_int64()
        self._check(lib().slideo_matcher_read_profile(self._h, ms, n, C.byref(pairs)))
        names = ["orb", "knn", "verify", "total"]
        return {names[i]: (ms[i], n[i]) for i in range(4)}, pairs.value

    def read_shader_clock(self):
        """-> (MHz the search kernel's waves ran at while profiling, blocks that recorded); clears the sums (ABI 7)."""
        mhz = C.c_double(); n = C.c_int64()
        self._check(lib().slideo_matcher_read_shader_clock(self._h, C.byref(mhz), C.byref(n)))
        return mhz.value, n.value

    # ---- frame mask (the setter: _FrameCalls) ----------------------------------------------
    @property
    def frame_mask_info(self):
        """(w, h) of the frame mask, or None."""
        w, h, on = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_matcher_frame_mask_info(self._h, C.byref(w), C.byref(h), C.byref(on)))
        return (w.value, h.value) if on.value else None

    def frame_mask_level(self, level):
        """Level `level` of the mask pyramid, uint8 [lh, lw] (the pyramid tap)."""
        lw, lh = C.c_int32(), C.c_int32()
        rc = lib().slideo_frame_mask_level(self._h, int(level), _p(np.empty(1, np.uint8)), C.c_int64(0), C.byref(lw), C.byref(lh))
        if rc not in (OK, 7):
            self._check(rc)
        out = np.empty((lh.value, lw.value), np.uint8)
        if out.size:
            self._check(lib().slideo_frame_mask_level(self._h, int(level), _p(out), C.c_int64(out.size), C.byref(lw), C.byref(lh)))
        return out

    # ---- debug taps -----------------------------------------------------------------
    def orb(self, bgr, cap=None):
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        cap = cap or 8192
        while True:
            kp = np.zeros(cap, KEYPOINT_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            n = C.c_int32()
            rc = lib().slideo_orb_bgr8(self._h, _p(bgr), w, h, w * 3, _p(kp), _p(desc), cap, C.byref(n))
            if rc == 7 and n.value > cap:                  # SLIDEO_ERR_CAPACITY: *n_out holds the number found
                cap = n.value
                continue
            self._check(rc)
            return kp[: n.value].copy(), desc[: n.value].copy()

    def pyramid_level(self, bgr, level, blurred):
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        out = np.empty(h * w, np.uint8)
        lw = C.c_int32(); lh = C.c_int32()
        self._check(lib().slideo_pyramid_level_bgr8(self._h, _p(bgr), w, h, w * 3, level, int(blurred), _p(out),
                                                    C.c_int64(out.size), C.byref(lw), C.byref(lh)))
        return out[: lw.value * lh.value].reshape(lh.value, lw.value).copy()

    def knn(self, q, t, k):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.uint16)
        self._check(lib().slideo_knn_hamming(self._h, _p(q), q.shape[0], _p(t), t.shape[0], k, _p(idx), _p(dist)))
        return idx, dist

    def l2_set_train(self, t):
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 128)
        self._check(lib().slideo_l2_set_train(self._h, _p(t), t.shape[0]))

    def l2_knn_dev(self, q_dev, nq, k, idx_dev, dist_dev):
        """device pointers in, device pointers out; returns the search kernels' HIP-event time in ms"""
        ms = C.c_float()
        self._check(lib().slideo_l2_knn_dev(self._h, C.c_void_p(q_dev), nq, k, C.c_void_p(idx_dev), C.c_void_p(dist_dev), C.byref(ms)))
        return ms.value

    def knn_lsh(self, q, t, k):
        """The LSH-compatible search (slideo_config.matcher 1) under this matcher's lsh_* parameters."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.uint16)
        self._check(lib().slideo_knn_lsh(self._h, _p(q), q.shape[0], _p(t), t.shape[0], k, _p(idx), _p(dist)))
        return idx, dist

    def knn_l2_u8(self, q, t, k):
        """Exact squared-L2 k-NN of 128-dim u8 descriptors on the matrix cores (north-star extension, see the header)."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 128)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 128)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.uint32)
        self._check(lib().slideo_knn_l2_u8(self._h, _p(q), q.shape[0], _p(t), t.shape[0], k, _p(idx), _p(dist)))
        return idx, dist

    def reduce(self, bgr, dw, dh):
        """cv::resize(bgr, (dw, dh), INTER_AREA) as the working-size reduce computes it (the reduce tap)."""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("expected an HxWx3 uint8 BGR image")
        h, w, _ = bgr.shape
        return self.reduce_pitched(bgr, w, h, w * 3, dw, dh)

    def reduce_pitched(self, buf, w, h, stride, dw, dh):
        """The same for an image of w x h in `buf` with rows `stride` bytes apart."""
        buf = np.ascontiguousarray(buf, np.uint8)
        out = np.empty((max(int(dh), 0), max(int(dw), 0), 3), np.uint8)
        self._check(lib().slideo_reduce_bgr8(self._h, _p(buf), int(w), int(h), int(stride), int(dw), int(dh), _p(out), C.c_int64(out.size)))
        return out

    def page_small_ssd(self, smalls):
        """slideo_page_small_ssd: smalls uint8 [n, sh, sw, 3] -> uint64 [n, page_count], the integer SSD of every small image with
        every deck page's (UINT64_MAX: a page of another small size).  The kernels and page operand of the direct page look-up."""
        smalls = np.ascontiguousarray(smalls, np.uint8)
        if smalls.ndim != 4 or smalls.shape[3] != 3:
            raise ValueError("expected [n, sh, sw, 3] uint8 small images")
        n, sh, sw, _ = smalls.shape
        out = np.empty((n, self.page_count), np.uint64)
        self._check(lib().slideo_page_small_ssd(self._h, _p(smalls), n, sw, sh, _p(out)))
        return out

    def page_small_ssd_valid(self, smalls):
        """slideo_page_small_ssd_valid: page_small_ssd over the valid pixels of the matcher's current validity map (a mask under
        MASK_GATE), whatever the direct similarity and scope are."""
        smalls = np.ascontiguousarray(smalls, np.uint8)
        if smalls.ndim != 4 or smalls.shape[3] != 3:
            raise ValueError("expected [n, sh, sw, 3] uint8 small images")
        n, sh, sw, _ = smalls.shape
        out = np.empty((n, self.page_count), np.uint64)
        self._check(lib().slideo_page_small_ssd_valid(self._h, _p(smalls), n, sw, sh, _p(out)))
        return out

    def small_gram_ssd(self, smalls, use_valid=False):
        """slideo_small_gram_ssd: smalls uint8 [n, sh, sw, 3] -> uint64 [n, n], the integer SSD of every pair of them (0 on the
        diagonal); use_valid: over the valid pixels of the matcher's current validity map.  The kernels of the gate reference
        'anchor'; needs no pages."""
        smalls = np.ascontiguousarray(smalls, np.uint8)
        if smalls.ndim != 4 or smalls.shape[3] != 3:
            raise ValueError("expected [n, sh, sw, 3] uint8 small images")
        n, sh, sw, _ = smalls.shape
        out = np.empty((n, n), np.uint64)
        self._check(lib().slideo_small_gram_ssd(self._h, _p(smalls), n, sw, sh, 1 if use_valid else 0, _p(out)))
        return out

    def small_carried_ssd(self, anchor_small, prev_small, smalls, use_valid=False):
        """slideo_small_carried_ssd: two small images [sh, sw, 3] and smalls uint8 [n, sh, sw, 3] -> uint64 [n + 1]: the integer SSD of
        anchor_small against every image, then of prev_small against image 0; prev_small None: uint64 [n], the first alone, as plain
        'anchor' launches it; use_valid: over the valid pixels of the matcher's current validity map.  The carried-SSD kernel of the
        gate reference 'anchor'; needs no pages."""
        smalls = np.ascontiguousarray(smalls, np.uint8)
        if smalls.ndim != 4 or smalls.shape[3] != 3 or len(smalls) < 1:
            raise ValueError("expected [n >= 1, sh, sw, 3] uint8 small images")
        n, sh, sw, _ = smalls.shape
        a = np.ascontiguousarray(anchor_small, np.uint8)
        p = np.ascontiguousarray(prev_small, np.uint8) if prev_small is not None else None
        if a.shape != smalls.shape[1:] or (p is not None and p.shape != smalls.shape[1:]):
            raise ValueError("anchor_small and prev_small have the small images' shape")
        out = np.empty(n + (p is not None), np.uint64)
        self._check(lib().slideo_small_carried_ssd(self._h, _p(a), _p(p), _p(smalls), n, sw, sh, 1 if use_valid else 0, _p(out)))
        return out

    def gate_settle_walk(self, dot, norm, carried, thr_c, thr_s, max_defer, d_in=0, none=False):
        """slideo_gate_settle_walk: dot [n, n] (<a'_i, a'_j>, read for i < j), norm int64 [n], carried uint64 [n + 1] ->
        (changed uint8 [n], ssd uint64 [n], last matched frame or -1, the deferral count behind the unit)."""
        norm = np.ascontiguousarray(norm, np.int64)
        n = len(norm)
        dot = np.ascontiguousarray(np.asarray(dot).astype(np.int64).view(np.uint64))
        carried = np.ascontiguousarray(carried, np.uint64)
        if dot.shape != (n, n) or carried.shape != (n + 1,):
            raise ValueError("expected dot [n, n], norm [n], carried [n + 1]")
        changed, ssd = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        a, d = C.c_int32(), C.c_int32()
        self._check(lib().slideo_gate_settle_walk(self._h, _p(dot), _p(norm), _p(carried), n, C.c_int64(int(thr_c)), C.c_int64(int(thr_s)),
                                                  int(max_defer), int(d_in), 1 if none else 0, _p(changed), _p(ssd), C.byref(a), C.byref(d)))
        return changed, ssd, a.value, d.value

    def gate_memory_entries(self):
        """slideo_matcher_gate_memory_entries -> (ordinals int64 [count], oldest first, the anchor's index among them or -1)."""
        count, anchor = C.c_int32(), C.c_int32()
        ords = np.zeros(GATE_MEMORY_MAX, np.int64)
        self._check(lib().slideo_matcher_gate_memory_entries(self._h, C.byref(count), C.byref(anchor), _p(ords)))
        return ords[:count.value].copy(), anchor.value

    def gate_memory_small(self, entry):
        """The small image [sh, sw, 3] of entry `entry` of the gate memory (0: the oldest), unmasked."""
        sw, sh = C.c_int32(), C.c_int32()
        out = np.empty(self.cfg.small_area * 3, np.uint8)
        self._check(lib().slideo_matcher_gate_memory_small(self._h, int(entry), _p(out), C.c_int64(out.size), C.byref(sw), C.byref(sh)))
        return out[:sw.value * sh.value * 3].reshape(sh.value, sw.value, 3).copy()

    def gate_recall_walk(self, dot, norm, mdot, mnorm, ordinals, count, head, anchor_slot, prev_ssd0, thr_c, thr_s, max_defer, d_in=0, none=False,
                         t0=0):
        """slideo_gate_recall_walk: dot [n, n] (read for i < j), norm int64 [n], mdot [n, M], mnorm int64 [M], the carried ring
        (ordinals int64 [M], count, head, anchor slot), frame 0's SSD against the carried previous frame ->
        (changed uint8 [n], ssd uint64 [n], refs int64 [n], occupants int32 [64], head, count, anchor slot, d)."""
        norm = np.ascontiguousarray(norm, np.int64)
        mnorm = np.ascontiguousarray(mnorm, np.int64)
        n, M = len(norm), len(mnorm)
        dot = np.ascontiguousarray(np.asarray(dot).astype(np.int64).view(np.uint64))
        mdot = np.ascontiguousarray(np.asarray(mdot).astype(np.int64).view(np.uint64))
        ordinals = np.ascontiguousarray(ordinals, np.int64)
        if dot.shape != (n, n) or mdot.shape != (n, M) or ordinals.shape != (M,):
            raise ValueError("expected dot [n, n], norm [n], mdot [n, M], mnorm [M], ordinals [M]")
        changed, ssd, refs = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.int64)
        occ = np.zeros(GATE_MEMORY_MAX, np.int32)
        h, c, a, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(lib().slideo_gate_recall_walk(
            self._h, _p(dot), _p(norm), _p(mdot), _p(mnorm), _p(ordinals), int(count), int(head), int(anchor_slot), C.c_uint64(int(prev_ssd0)), n, M,
            C.c_int64(int(thr_c)), C.c_int64(int(thr_s)), int(max_defer), int(d_in), 1 if none else 0, C.c_int64(int(t0)), _p(changed), _p(ssd),
            _p(refs), _p(occ), C.byref(h), C.byref(c), C.byref(a), C.byref(d)))
        return changed, ssd, refs, occ, h.value, c.value, a.value, d.value

    def small_image(self, bgr):
        bgr = _img3(bgr)
        h, w, _ = bgr.shape
        sw, sh = small_size(w, h, self.cfg.small_area)
        out = np.empty((max(sh, 1), max(sw, 1), 3), np.uint8)
        a = C.c_int32(); b = C.c_int32()
        self._check(lib().slideo_small_image_bgr8(self._h, _p(bgr), w, h, w * 3, _p(out), C.c_int64(out.size),
                                                  C.byref(a), C.byref(b)))
        return out

    def match_features(self, frames, kps, descs):
        """slideo_match_frames_features_bgr8 (debug tap): match_frames from the frames' features on.  frames: uint8 [n, h, w, 3];
        kps / descs: per frame a KEYPOINT_DTYPE array and its uint8 [k, 32] descriptors, in place of ORB's output -> verdict records
        (last_candidates works after it)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w, c = frames.shape
        assert c == 3 and len(kps) == n and len(descs) == n
        kps = [np.ascontiguousarray(k, KEYPOINT_DTYPE).reshape(-1) for k in kps]
        descs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descs]
        assert all(len(k) == len(d) for k, d in zip(kps, descs))
        counts = np.array([len(k) for k in kps], np.int32)
        kp = np.ascontiguousarray(np.concatenate(kps)) if n else np.zeros(0, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(np.concatenate(descs)) if n else np.zeros((0, 32), np.uint8)
        out = np.zeros(n, VERDICT_DTYPE)
        self._check(lib().slideo_match_frames_features_bgr8(self._h, n, _p(frames), w, h, w * 3, C.c_int64(w * h * 3), _p(counts),
                                                            _p(kp), _p(desc), _p(out)))
        return out


class Group(_FrameCalls):
    """slideo_group (include/slideo_amd.h, "N-device group"): one matcher per device behind one handle — page DB replicated,
    a call's pages and frames sharded contiguously over the devices, verdicts gathered into one host array.  Results equal
    a single Matcher's bit for bit.  `devices`: HIP ordinals (may repeat); None or empty = every gfx950 device of the node."""
    _PREFIX = "slideo_group_"
    _SETS = "slideo_group_"

    def __init__(self, cfg=None, devices=None):
        self.cfg = cfg if cfg is not None else default_config()
        self._h = C.c_void_p()
        self._cb = None
        if devices is None or len(devices) == 0:     # (an empty list = n_devices 0 = the same request: never a stale empty self.devices)
            # every gfx950 device of the node: the library enumerates them by their own HIP ordinals (n_devices 0)
            rc = lib().slideo_group_create(C.byref(self.cfg), 0, None, C.byref(self._h))
            self.devices = device_list() if rc == OK else []
        else:
            self.devices = [int(d) for d in devices]
            arr = (C.c_int32 * len(self.devices))(*self.devices)
            rc = lib().slideo_group_create(C.byref(self.cfg), len(self.devices), arr, C.byref(self._h))
        if rc != OK:
            raise SlideoError(rc, lib().slideo_group_last_error(None).decode())

    def _check(self, rc):
        if rc != OK:
            raise SlideoError(rc, lib().slideo_group_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().slideo_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def member(self, i):
        """Member i as a (non-owning) Matcher: introspection, taps, profiling."""
        m = Matcher.__new__(Matcher)
        m.cfg, m._cb = self.cfg, None
        m._h = C.c_void_p(lib().slideo_group_member(self._h, int(i)))
        m.close = lambda: None                       # the group owns the handle
        if getattr(self, "_sift", False):
            m._sift = True
        return m

    def set_progress(self, fn):
        if fn is None:
            self._cb = None
            self._check(lib().slideo_group_set_progress(self._h, None, None))
            return
        self._cb = PROGRESS_FN(lambda user, d, t, msg: fn(int(d), int(t), (msg or b"").decode()))
        self._check(lib().slideo_group_set_progress(self._h, self._cb, None))

    def use_sift(self, sift_cfg, ratio=0.0):
        self._check(lib().slideo_group_use_sift(self._h, C.byref(sift_cfg), C.c_float(ratio)))
        self._sift = True

    def add_pages(self, pages):
        pages = [_img3(p) for p in pages]
        n = len(pages)
        ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in pages])
        w = (C.c_int32 * n)(*[p.shape[1] for p in pages])
        h = (C.c_int32 * n)(*[p.shape[0] for p in pages])
        s = (C.c_int32 * n)(*[p.shape[1] * 3 for p in pages])
        self._check(lib().slideo_group_add_pages_bgr8(self._h, n, ptrs, w, h, s))

    def finalize(self):
        self._check(lib().slideo_group_finalize_pages(self._h))

    @property
    def page_count(self):
        return int(lib().slideo_group_page_count(self._h))

    @property
    def descriptor_count(self):
        return int(lib().slideo_group_descriptor_count(self._h))

    def page_set_info(self, set_id):
        """Member 0's record of set `set_id` (every member holds the same set)."""
        return self.member(0).page_set_info(set_id)

    # ---- group gate order (include/slideo_amd.h "Group gate order") --------------------------------------------------------------
    def set_gate_order(self, order):
        """ "halo" (the default: a later shard is primed from one frame) or "chain" (every shard receives its predecessor's whole gate
        state: ANCHOR and a gate settle run on any member count); or the GROUP_GATE_* value.  Resets the gate state."""
        if isinstance(order, str):
            if order not in GROUP_GATE_ORDERS:
                raise SlideoError(1, "group gate order %r: one of %s" % (order, sorted(GROUP_GATE_ORDERS)))
            order = GROUP_GATE_ORDERS[order]
        if not 0 <= int(order) <= 0xFFFFFFFF:
            raise SlideoError(1, "group gate order %r" % (order,))
        self._check(lib().slideo_group_set_gate_order(self._h, int(order)))

    def gate_order(self):
        v = C.c_uint32()
        self._check(lib().slideo_group_gate_order(self._h, C.byref(v)))
        return {b: a for a, b in GROUP_GATE_ORDERS.items()}[int(v.value)]

    def gate_chain_waited(self, member):
        """Seconds member `member` (>= 1) blocked for its predecessor's gate state in the last chained gated call."""
        s = C.c_double()
        self._check(lib().slideo_group_gate_chain_waited(self._h, int(member), C.byref(s)))
        return float(s.value)


def device_count():
    """gfx950 devices visible to this process."""
    return int(lib().slideo_device_count())


def device_list():
    """Their HIP ordinals (not necessarily 0 .. count-1 on a node that also holds other architectures)."""
    n = int(lib().slideo_device_list(None, 0))
    arr = (C.c_int32 * max(n, 1))()
    n = min(n, int(lib().slideo_device_list(arr, n)))
    return [int(arr[i]) for i in range(n)]


def _evidence_arrays(seen, hit):
    seen, hit = np.ascontiguousarray(seen, np.uint32), np.ascontiguousarray(hit, np.uint32)
    if seen.ndim != 2 or seen.shape != hit.shape:
        raise ValueError("seen and hit: two uint32 [gh, gw] arrays, got %s and %s" % (seen.shape, hit.shape))
    return seen, hit, seen.shape[1], seen.shape[0]


def evidence_mask(seen, hit, cell, aw, ah, min_seen, min_hit, grow):
    """slideo_evidence_mask (include/slideo_amd.h "Match evidence map"): min_hit a float in [0, 1], rounded to parts per million ->
    mask uint8 [ah, aw] of 0 / 255, what set_frame_mask takes."""
    seen, hit, gw, gh = _evidence_arrays(seen, hit)
    out = np.empty((max(int(ah), 0), max(int(aw), 0)), np.uint8)
    rc = lib().slideo_evidence_mask(_p(seen), _p(hit), gw, gh, int(cell), int(aw), int(ah), C.c_int64(int(min_seen)),
                                    int(round(float(min_hit) * 1000000)), int(grow), _p(out) if out.size else None, C.c_int64(int(aw)))
    if rc != OK:
        raise SlideoError(rc, "slideo_evidence_mask: an argument outside its range (include/slideo_amd.h \"Match evidence map\")")
    return out


def evidence_box(seen, hit, cell, aw, ah, min_hits, min_hit):
    """slideo_evidence_box: -> (x0, y0, x1, y1), x1 and y1 exclusive; all -1 when no cell qualifies."""
    seen, hit, gw, gh = _evidence_arrays(seen, hit)
    box = (C.c_int32 * 4)()
    rc = lib().slideo_evidence_box(_p(seen), _p(hit), gw, gh, int(cell), int(aw), int(ah), C.c_int64(int(min_hits)),
                                   int(round(float(min_hit) * 1000000)), box)
    if rc != OK:
        raise SlideoError(rc, "slideo_evidence_box: an argument outside its range (include/slideo_amd.h \"Match evidence map\")")
    return tuple(box)


def tone_lut(cnt, sm, min_count):
    """slideo_tone_lut (include/slideo_amd.h "Match tone table"): cnt, sm uint64 [3, 256] -> the table uint8 [3, 256], what
    set_frame_levels takes.  SlideoError: min_count < 1, or a channel in which no frame value was seen min_count times."""
    cnt, sm = np.ascontiguousarray(cnt, np.uint64), np.ascontiguousarray(sm, np.uint64)
    if cnt.shape != (3, 256) or sm.shape != (3, 256):
        raise ValueError("cnt and sum: two uint64 [3, 256] arrays, got %s and %s" % (cnt.shape, sm.shape))
    out = np.zeros((3, 256), np.uint8)
    rc = lib().slideo_tone_lut(_p(cnt), _p(sm), C.c_int64(int(min_count)), _p(out))
    if rc != OK:
        raise SlideoError(rc, "slideo_tone_lut: min_count below 1, a channel without an anchor, or counts no session gives "
                              "(include/slideo_amd.h \"Match tone table\")")
    return out


def placement_quad(sums, cell, aw, ah, min_count, trim_px, rounds):
    """slideo_placement_quad (include/slideo_amd.h "Match placement map"): sums uint64 [5, gh, gw] (n, sfx, sfy, su, sv) -> (quad
    [(x, y)] * 4 top-left, top-right, bottom-right, bottom-left in pixels of the analysed image, H float64 [3, 3], cells_used,
    rms_px).  SlideoError: an argument outside its range, fewer than 4 cells with min_count keypoints at a stage, or cells that do
    not determine a homography."""
    sums = np.ascontiguousarray(sums, np.uint64)
    if sums.ndim != 3 or sums.shape[0] != 5:
        raise ValueError("sums: one uint64 [5, gh, gw] array, got %s" % (sums.shape,))
    quad, H = np.zeros(8, np.float64), np.zeros(9, np.float64)
    used, rms = C.c_int32(), C.c_double()
    rc = lib().slideo_placement_quad(*[_p(sums[i]) for i in range(5)], sums.shape[2], sums.shape[1], int(cell), int(aw), int(ah),
                                     C.c_int64(int(min_count)), C.c_double(float(trim_px)), int(rounds), _p(quad), _p(H), C.byref(used), C.byref(rms))
    if rc != OK:
        raise SlideoError(rc, "slideo_placement_quad: an argument outside its range, fewer than 4 cells of min_count keypoints, or cells "
                              "that determine no homography (include/slideo_amd.h \"Match placement map\")")
    return [(float(quad[2 * i]), float(quad[2 * i + 1])) for i in range(4)], H.reshape(3, 3), used.value, rms.value


def frame_lens_defaults(src_w, src_h, cx=None, cy=None, f=None):
    """The mirrors' defaults of "Frame lens": the image centre and half the source diagonal."""
    cx = (src_w - 1) / 2.0 if cx is None else cx
    cy = (src_h - 1) / 2.0 if cy is None else cy
    f = 0.5 * float(np.hypot(src_w, src_h)) if f is None else f
    return float(cx), float(cy), float(f)


def frame_lens_point(cx, cy, f, k1, k2, u, v):
    """slideo_frame_lens_point: where the camera sees the ideal point (u, v) under the lens -> (xd, yd).  A pure host function."""
    xd, yd = C.c_double(), C.c_double()
    rc = lib().slideo_frame_lens_point(float(cx), float(cy), float(f), float(k1), float(k2), float(u), float(v), C.byref(xd), C.byref(yd))
    if rc != OK:
        raise SlideoError(rc, "slideo_frame_lens_point: a non-finite argument or f <= 0")
    return xd.value, yd.value


def placement_lens(sums, cell, aw, ah, min_count, cx, cy, f, order, trim_px, rounds, iters):
    """slideo_placement_lens (include/slideo_amd.h "Placement lens"): sums uint64 [5, gh, gw] of a placement session that ran with no
    lens and no region -> ((k1, k2), quad [(x, y)] * 4 in IDEAL pixels, H float64 [3, 3] unit slide -> ideal pixels, cells_used,
    rms_px).  SlideoError: an argument outside its range, too few cells at a stage, cells that do not determine the fit, or a fit
    whose radial map is not increasing over the kept cells."""
    sums = np.ascontiguousarray(sums, np.uint64)
    if sums.ndim != 3 or sums.shape[0] != 5:
        raise ValueError("sums: one uint64 [5, gh, gw] array, got %s" % (sums.shape,))
    k, quad, H = np.zeros(2, np.float64), np.zeros(8, np.float64), np.zeros(9, np.float64)
    used, rms = C.c_int32(), C.c_double()
    rc = lib().slideo_placement_lens(*[_p(sums[i]) for i in range(5)], sums.shape[2], sums.shape[1], int(cell), int(aw), int(ah),
                                     C.c_int64(int(min_count)), float(cx), float(cy), float(f), int(order), float(trim_px), int(rounds), int(iters),
                                     _p(k), _p(quad), _p(H), C.byref(used), C.byref(rms))
    if rc != OK:
        raise SlideoError(rc, "slideo_placement_lens: an argument outside its range, fewer than 4 + order cells of min_count keypoints, cells "
                              "that determine no fit, or a radial map that is not increasing (include/slideo_amd.h \"Placement lens\")")
    return (float(k[0]), float(k[1])), [(float(quad[2 * i]), float(quad[2 * i + 1])) for i in range(4)], H.reshape(3, 3), used.value, rms.value


def changed_ssd_threshold(changed_similarity, small_w, small_h):
    """The smallest SSD of two small_w x small_h small images that counts as changed (slideo_changed_ssd_threshold; a host rule).
    2**63 - 1: no SSD does."""
    t = int(lib().slideo_changed_ssd_threshold(C.c_float(changed_similarity), int(small_w), int(small_h)))
    if t < 0:
        raise SlideoError(1, "changed_ssd_threshold: bad small-image size %rx%r" % (small_w, small_h))
    return t


def direct_ssd_threshold(t, n_pixels):
    """slideo_direct_ssd_threshold: the largest SSD of two small images of n_pixels pixels whose similarity is >= t (-1: bad
    arguments, or none)."""
    return int(lib().slideo_direct_ssd_threshold(C.c_float(t), C.c_int64(int(n_pixels))))


def changed_ssd_threshold_n(changed_similarity, n_pixels):
    """slideo_changed_ssd_threshold_n: the smallest changed SSD when the similarity is normalised over n_pixels pixels (the n_valid
    of the frame mask's GATE scope)."""
    t = int(lib().slideo_changed_ssd_threshold_n(C.c_float(changed_similarity), C.c_int64(int(n_pixels))))
    if t < 0:
        raise SlideoError(1, "changed_ssd_threshold_n: bad pixel count %r" % (n_pixels,))
    return t


def frame_region_from_quad(quad, out_w, out_h):
    """slideo_frame_region_from_quad: the 3x3 map (float64 [3, 3]) that takes the corners of the out_w x out_h image onto `quad` —
    the source coordinates of the slide's top-left, top-right, bottom-right and bottom-left corner.  A pure host function."""
    q = np.ascontiguousarray(np.asarray(quad, np.float64).reshape(-1))
    if q.size != 8:
        raise SlideoError(1, "frame_region_from_quad: expected 4 (x, y) corners")
    M = np.zeros(9, np.float64)
    rc = lib().slideo_frame_region_from_quad(_p(q), int(out_w), int(out_h), _p(M))
    if rc != OK:
        raise SlideoError(rc, "slideo_frame_region_from_quad: a degenerate or non-convex quad, or an output size outside 2..4096")
    return M.reshape(3, 3)


def working_size(w, h, max_w, max_h):
    """slideo_working_size: the size a w x h frame stands for under the working size (max_w, max_h) — (w, h) when it fits."""
    dw, dh = C.c_int32(), C.c_int32()
    rc = lib().slideo_working_size(int(w), int(h), int(max_w), int(max_h), C.byref(dw), C.byref(dh))
    if rc != OK:
        raise SlideoError(rc, "slideo_working_size(%d, %d, %d, %d)" % (w, h, max_w, max_h))
    return dw.value, dh.value


def small_size(w, h, small_area=120000):
    """to_small_image target size (crates/matching-opencv/src/image_utils.rs:11-16), f32 arithmetic."""
    factor = np.sqrt(np.float32(small_area) / np.float32(w * h), dtype=np.float32)
    return int(np.float32(w) * factor), int(np.float32(h) * factor)
