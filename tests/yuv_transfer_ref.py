"""Test-side numpy restatement of include/slideo_amd.h "YUV transfer": steps 1-5 over the integers slideo_yuv_transfer_tables
returns (the library's tables are the definition), the header's formulas for those tables in float64 (what the tables are held to),
and a float64 forward transform (sRGB BGR -> linear -> BT.2020 -> nits at white_nits -> OETF -> 10-bit Y'CbCr) the tests make
HDR frames with.  Written from the header, not from csrc/.  Layouts, sizes and sample offsets come from tests/yuv_desc_ref.py,
tests/yuv_sampling_ref.py and tests/yuv_chroma_ref.py by import.  `layout`: anything with the fields of slideo_yuv420_layout;
strides and offsets are BYTES."""
import numpy as np

import yuv_chroma_ref as CR
import yuv_desc_ref as D
import yuv_sampling_ref as S

SDR, HLG, PQ = 0, 1, 2
TRANSFER_NAMES = {SDR: "sdr", HLG: "hlg", PQ: "pq"}
LIMITED, FULL = D.LIMITED, D.FULL
D10_MSB, D10_LSB = D.D10_MSB, D.D10_LSB
DEPTHS = (D10_MSB, D10_LSB)
DEPTH_NAMES = {D10_MSB: "10_msb", D10_LSB: "10_lsb"}
S420, S422, S444 = S.S420, S.S422, S.S444
SAMPLINGS = (S420, S422, S444)
SAMPLING_NAMES = S.SAMPLING_NAMES
FORMATS = {S420: D.FORMATS, S422: S.FORMATS[S422], S444: S.FORMATS[S444]}
PAIRS = [(t, r) for t in (HLG, PQ) for r in (LIMITED, FULL)]
# the header's integers, written out
COEF_LIMITED = (306134, 563104, -49251, -171006, 441349, 64, 18)
COEF_FULL = (262144, 493198, -43137, -149777, 386558, 0, 18)
GAMUT = ((27206, -9628, -1194), (-2041, 18562, -137), (-297, -1648, 18329))
KR, KB = 0.2627, 0.0593
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


# ---- the header's formulas in float64 (unrounded) -----------------------------------------------------------------------------------
def nits(transfer, e):
    e = np.asarray(e, np.float64)
    if transfer == PQ:
        p = e ** (1.0 / PQ_M2)
        return 10000.0 * (np.maximum(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p)) ** (1.0 / PQ_M1)
    E = np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)
    return 1000.0 * E ** 1.2


def signal(transfer, n):
    """The inverse of nits(): the signal e in 0..1 of display light n (the forward model's OETF side)."""
    n = np.asarray(n, np.float64)
    if transfer == PQ:
        y = (n / 10000.0) ** PQ_M1
        return ((PQ_C1 + PQ_C2 * y) / (1.0 + PQ_C3 * y)) ** PQ_M2
    E = (n / 1000.0) ** (1.0 / 1.2)
    return np.where(E <= 1.0 / 12.0, np.sqrt(3.0 * E), HLG_A * np.log(np.maximum(12.0 * E - HLG_B, 1e-300)) + HLG_C)


def white(white_nits):
    return 203.0 if white_nits == 0 else float(white_nits)


def lin_formula(transfer, white_nits):
    return 16383.0 * np.minimum(1.0, nits(transfer, np.arange(1024) / 1023.0) / white(white_nits))


def srgb_oetf(l):
    l = np.asarray(l, np.float64)
    return np.where(l <= 0.0031308, 12.92 * l, 1.055 * l ** (1.0 / 2.4) - 0.055)


def srgb_eotf(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def out_formula():
    return 255.0 * srgb_oetf(np.arange(4096) / 4095.0)


def rgb_to_xyz(prim):
    """RGB -> XYZ of primaries ((xr, yr), (xg, yg), (xb, yb)) under D65 (0.3127, 0.3290)."""
    P = np.array([[x / y for x, y in prim], [1.0, 1.0, 1.0], [(1.0 - x - y) / y for x, y in prim]], np.float64)
    W = np.array([0.3127 / 0.3290, 1.0, (1.0 - 0.3127 - 0.3290) / 0.3290])
    return P * np.linalg.solve(P, W)[None, :]


def gamut_float():
    """G = M709^-1 M2020."""
    m709 = rgb_to_xyz(((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)))
    m2020 = rgb_to_xyz(((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)))
    return np.linalg.solve(m709, m2020)


def coef_formula(rng):
    """The seven integers of step 2 by the header's rule (unrounded floats for the five coefficients)."""
    Kg = 1.0 - KR - KB
    sy, sc = (1.0, 1.0) if rng == FULL else (1023.0 / 876.0, 1023.0 / 896.0)
    one = float(1 << 18)
    return (sy * one, sc * 2 * (1 - KB) * one, -(sc * 2 * (1 - KB) * KB / Kg * one), -(sc * 2 * (1 - KR) * KR / Kg * one), sc * 2 * (1 - KR) * one,
            0 if rng == FULL else 64, 18)


# ---- the library's integers -----------------------------------------------------------------------------------------------------------
class Tables:
    def __init__(self, coef, gamut, lin, out):
        self.coef = [int(x) for x in coef]
        self.gamut = np.asarray(gamut, np.int64).reshape(3, 3)
        self.lin = np.asarray(lin, np.int64)
        self.out = np.asarray(out, np.int64)


def tables(capi, transfer, rng, white_nits=0):
    return Tables(*capi.yuv_transfer_tables(transfer, rng, white_nits))


# ---- steps 1-5 -------------------------------------------------------------------------------------------------------------------------
def s10(raw, depth):
    return raw >> 6 if depth == D10_MSB else np.minimum(raw, 1023)


def sample_offsets(w, h, layout, depth, sampling):
    return CR.sample_offsets(w, h, layout, depth, sampling)


def codes(buf, w, h, layout, T, depth, sampling):
    """Steps 1 and 2: the R'G'B' codes [h, w, 3] (R, G, B order), 0..1023."""
    CY, CUB, CUG, CVG, CVR, yofs, shift = T.coef
    half = 1 << (shift - 1)
    oy, ou, ov = sample_offsets(w, h, layout, depth, sampling)
    Y, U, V = (s10(D.samples(buf, o, depth), depth) for o in (oy, ou, ov))
    if sampling == S420:
        U, V = (np.repeat(np.repeat(c, 2, 0), 2, 1) for c in (U, V))
    elif sampling == S422:
        U, V = np.repeat(U, 2, 1), np.repeat(V, 2, 1)
    u, v = U - 512, V - 512
    y = np.maximum(Y - yofs, 0) * CY
    r = (y + half + CVR * v) >> shift
    g = (y + half + CVG * v + CUG * u) >> shift
    b = (y + half + CUB * u) >> shift
    return np.clip(np.stack([r, g, b], -1), 0, 1023)


def to_bgr(buf, w, h, layout, T, depth, sampling):
    """The BGR8 image [h, w, 3] one frame stands for under the tables T (of a transfer, a range and white_nits)."""
    lin = T.lin[codes(buf, w, h, layout, T, depth, sampling)]                # [h, w, 3] R G B
    o = np.clip((lin @ T.gamut.T + (1 << 13)) >> 14, 0, 16383)
    byte = T.out[np.minimum(4095, (o + 2) >> 2)]
    return byte[..., ::-1].astype(np.uint8)


def frames_to_bgr(yuv, w, h, layout, T, depth, sampling):
    return np.stack([to_bgr(f, w, h, layout, T, depth, sampling) for f in yuv])


# ---- the forward direction (an encoder's side: its exact rounding is not part of any contract) ----------------------------------------
def from_bgr(bgr, transfer, rng, white_nits, sampling):
    """A BGR8 image [h, w, 3] -> 10-bit (Y, U, V) values as floats (unrounded); chroma the mean of the pixels that share a sample."""
    f = np.asarray(bgr, np.float64) / 255.0
    lin709 = srgb_eotf(f[..., ::-1])                                         # R G B
    lin2020 = np.clip(lin709 @ np.linalg.inv(gamut_float()).T, 0.0, None)
    e = signal(transfer, lin2020 * white(white_nits))
    r, g, b = e[..., 0], e[..., 1], e[..., 2]
    y = KR * r + (1.0 - KR - KB) * g + KB * b
    cb, cr = (b - y) / (2.0 * (1.0 - KB)), (r - y) / (2.0 * (1.0 - KR))
    if rng == FULL:
        Y, U, V = 1023.0 * y, 512.0 + 1023.0 * cb, 512.0 + 1023.0 * cr
    else:
        Y, U, V = 64.0 + 876.0 * y, 512.0 + 896.0 * cb, 512.0 + 896.0 * cr
    if sampling == S420:
        U, V = (c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3)) for c in (U, V))
    elif sampling == S422:
        U, V = (c.reshape(c.shape[0], c.shape[1] // 2, 2).mean(axis=2) for c in (U, V))
    return Y, U, V


def quantise(plane, depth):
    v10 = np.clip(np.rint(plane), 0, 1023).astype(np.int64)
    return v10 << 6 if depth == D10_MSB else v10


def pack(Y, U, V, w, h, layout, frame_bytes, depth, sampling, seed=0):
    """One frame's bytes from RAW container values; the bytes no sample covers are random."""
    if sampling == S420:
        return D.pack(Y, U, V, w, h, layout, frame_bytes, depth, seed)
    return S.pack(Y, U, V, w, h, layout, frame_bytes, depth, sampling, seed)


def frames_to_yuv(frames, layout, frame_bytes, transfer, rng, depth, sampling=S420, white_nits=0):
    """[n, h, w, 3] sRGB BGR frames -> [n, frame_bytes] HDR frames of `sampling` in `layout`."""
    out = []
    for f in frames:
        h, w = f.shape[:2]
        Y, U, V = from_bgr(f, transfer, rng, white_nits, sampling)
        out.append(pack(quantise(Y, depth), quantise(U, depth), quantise(V, depth), w, h, layout, frame_bytes, depth, sampling))
    return np.stack(out)


# ---- the conversion cases the CPU host check and the GPU tap test share -------------------------------------------------------------
SPECIALS = (0, 64, 512, 940, 960, 1023)


def sizes(sampling):
    """4:2:0: yuv_desc_ref's (2, 2) .. (130, 70); 4:2:2 / 4:4:4: yuv_sampling_ref's lists with their ragged tails and odd heights."""
    return list(D.SIZES) if sampling == S420 else S.sizes(sampling)


def layouts(capi, fmt, w, h, depth):
    """[(name, layout, frame bytes)]: tight, pitched (every wide load applies) and skewed (they miss), by the sampling's own rules
    (yuv_chroma_ref.layouts: yuv_desc_ref's with skewed2 for interleaved 4:2:0, yuv_sampling_ref's otherwise)."""
    return CR.layouts(capi, fmt, w, h, depth)


def random_frame(w, h, layout, frame_bytes, depth, sampling, seed):
    """Raw 10-bit values uniform over 0..1023 with SPECIALS sprinkled in; 10_MSB: random low 6 bits under the value; 10_LSB: a share
    of containers above 1023."""
    rng = np.random.default_rng(seed)

    def plane(ph, pw):
        v = rng.integers(0, 1024, (ph, pw), dtype=np.int64)
        pick = rng.random((ph, pw)) < 0.3
        v[pick] = np.asarray(SPECIALS, np.int64)[rng.integers(0, len(SPECIALS), int(pick.sum()))]
        if depth == D10_MSB:
            v = (v << 6) | rng.integers(0, 64, (ph, pw), dtype=np.int64)
        else:
            over = rng.random((ph, pw)) < 0.1
            v[over] = rng.integers(1024, 65536, int(over.sum()), dtype=np.int64)
        return v
    cw, chh = (w // 2, h // 2) if sampling == S420 else (w // 2, h) if sampling == S422 else (w, h)
    return pack(plane(h, w), plane(chh, cw), plane(chh, cw), w, h, layout, frame_bytes, depth, sampling, seed)


def special_frame(w, h, layout, frame_bytes, depth, sampling):
    """Every plane cycles through SPECIALS (10_LSB: with one container above 1023 in the cycle), the three planes out of step."""
    vals = np.asarray(SPECIALS + ((40000,) if depth == D10_LSB else ()), np.int64)

    def plane(ph, pw, mul, off):             # (mul is coprime to 6 and to 7: every value occurs)
        v = vals[(np.arange(ph * pw) * mul + off) % len(vals)].reshape(ph, pw)
        return v << 6 if depth == D10_MSB else v
    cw, chh = (w // 2, h // 2) if sampling == S420 else (w // 2, h) if sampling == S422 else (w, h)
    return pack(plane(h, w, 1, 0), plane(chh, cw, 5, 1), plane(chh, cw, 1, 3), w, h, layout, frame_bytes, depth, sampling, 1)


def tap_cases(capi):
    """Every (sampling, depth, fmt, layout name, layout, frame bytes, w, h) of the matrix; the transfer, the range and white_nits
    rotate over them in the caller."""
    for sampling in SAMPLINGS:
        for depth in DEPTHS:
            for fmt in FORMATS[sampling]:
                for (w, h) in sizes(sampling):
                    for name, L, fb in layouts(capi, fmt, w, h, depth):
                        yield sampling, depth, fmt, name, L, fb, w, h


NITS = (0, 100, 1000)


def pick(k):
    """The (transfer, range, white_nits) of case k."""
    t, r = PAIRS[k % 4]
    return t, r, NITS[(k // 4) % 3]
