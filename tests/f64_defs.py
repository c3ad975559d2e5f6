"""Test-side float64 definitions of the ORB and re-projection steps (mo/feature_extractor.rs, mo/image_utils.rs, mo/lib.rs; mo/ =
crates/matching-opencv/src/ of the reference), written from the published algorithms, not from oracle/ or the kernels.

Plain numpy, float64 or exact integers.  Nothing here imports the restatement or the product.  The only inputs taken from
outside are the ORB configuration literals and the BRIEF point pattern (a constant table; tests/test_oracle_constants.py pins
its hash), and both are passed in as arguments.  tests/test_oracle_f64_definitions.py holds the CPU restatement to these
definitions and tests/test_gpu_f64_definitions.py the HIP kernels."""
import numpy as np

# FAST's Bresenham circle of radius 3, in order around the centre (dx, dy)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))

BRIEF_MARGIN = 1e-4            # a rotated BRIEF coordinate this close to a half-integer may round either way
WARP_MARGIN = 2.0 ** -9        # warpAffine's 10-bit fixed point (error <= 2^-10) plus an f32 coordinate at 4K (ulp 2^-11)
PERSP_MARGIN = 2.0 ** -20      # warpPerspective maps in f64 (imgwarp.cpp WarpPerspectiveInvoker): only f64 round-off, < 1e-9
F32_U = 2.0 ** -24             # unit round-off of f32
AREA_CUTOFF = 1e-3             # computeResizeAreaTab drops an edge cell whose overlap is at most this


def gray(bgr):
    """cvtColor(BGR2GRAY) (feature_extractor.rs: ORB's detectAndCompute converts the frame): 0.114 B + 0.587 G + 0.299 R,
    unrounded."""
    f = np.asarray(bgr, np.float64)
    return 0.114 * f[..., 0] + 0.587 * f[..., 1] + 0.299 * f[..., 2]


def level_scales(scale_factor, nlevels):
    """ORB's getScale: the f32 of scaleFactor^level (scaleFactor is the f32 ORB argument, feature_extractor.rs)."""
    sf = float(np.float32(scale_factor))
    return np.array([np.float32(sf ** l) for l in range(nlevels)], np.float32)


def level_sizes(w, h, scale_factor, nlevels):
    """ORB's pyramid (feature_extractor.rs -> orb.cpp detectAndCompute): level l is cvRound(side / scale_l), the division in f32.
    -> (widths, heights, scales)."""
    s = level_scales(scale_factor, nlevels)
    ws = np.rint(np.float32(w) / s).astype(np.int64)
    hs = np.rint(np.float32(h) / s).astype(np.int64)
    return ws, hs, s


def level_quotas(nfeatures, scale_factor, nlevels):
    """ORB's per-level feature quotas (orb.cpp computeKeyPoints): ndesired = n (1 - f) / (1 - f^nlevels) with f = 1 / scaleFactor,
    level l gets cvRound(ndesired f^l), all in f32; the last level gets what is left (never below 0)."""
    f32 = np.float32
    factor = f32(1.0 / float(f32(scale_factor)))
    nd = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** nlevels))
    q = []
    for _ in range(nlevels - 1):
        q.append(int(np.rint(nd)))
        nd = f32(nd * factor)
    q.append(max(nfeatures - sum(q), 0))
    return np.array(q, np.int64)


def _lin_axis(s, d):
    f = (np.arange(d) + 0.5) * (s / d) - 0.5                 # half-pixel centres
    i0 = np.floor(f)
    a = f - i0
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, s - 1), np.clip(i0 + 1, 0, s - 1), a


def bilinear_down(img, dw, dh):
    """One pyramid step, resize(INTER_LINEAR) (orb.cpp builds level l from level l - 1): the source position of destination
    pixel d is (d + 0.5) s / d' - 0.5, the two neighbours are clamped to the image (edge replicate), bilinear weights, float64."""
    f = np.asarray(img, np.float64)
    y0, y1, ay = _lin_axis(f.shape[0], dh)
    x0, x1, ax = _lin_axis(f.shape[1], dw)
    r = f[y0] * (1 - ay)[:, None] + f[y1] * ay[:, None]
    return r[:, x0] * (1 - ax)[None, :] + r[:, x1] * ax[None, :]


def bilinear_q8_bound(img, dw, dh):
    """How far resize(INTER_LINEAR_EXACT) (8.8 fixed-point weights, exact integer sums, one rounding of the 16-bit fraction) may
    lie from bilinear_down, per destination pixel.  Derivation: each axis weight c / 256 is within 1/512 of the exact one and
    both weight pairs sum to 1, so a row's fixed-point interpolation errs by at most |p1 - p0| / 512, the column blend of the two
    rows adds at most |r1 - r0| / 512 (r = the exact row values), and the final rounding 0.5:
    0.5 + (max over the two rows |p1 - p0| + |r1 - r0|) / 512."""
    f = np.asarray(img, np.float64)
    y0, y1, ay = _lin_axis(f.shape[0], dh)
    x0, x1, ax = _lin_axis(f.shape[1], dw)
    rows = [f[y][:, x0] * (1 - ax)[None, :] + f[y][:, x1] * ax[None, :] for y in (y0, y1)]
    dx = np.maximum(np.abs(f[y0][:, x1] - f[y0][:, x0]), np.abs(f[y1][:, x1] - f[y1][:, x0]))
    return 0.5 + (dx + np.abs(rows[1] - rows[0])) / 512.0 + 1e-9


def gauss7(img, sigma=2.0):
    """GaussianBlur(7x7, sigma 2) of each level before BRIEF (orb.cpp computeKeyPoints): separable, taps exp(-x^2 / 2 sigma^2)
    normalised to sum 1, BORDER_REFLECT_101 (numpy's "reflect"), float64, unrounded."""
    x = np.arange(-3, 4, dtype=np.float64)
    k = np.exp(-x * x / (2.0 * sigma * sigma))
    k /= k.sum()
    f = np.asarray(img, np.float64)
    h, w = f.shape
    p = np.pad(f, 3, mode="reflect")
    t = sum(k[i] * p[:, i:i + w] for i in range(7))
    return sum(k[i] * t[i:i + h, :] for i in range(7))


def fast_score(img, t):
    """FAST-9/16 with its score (orb.cpp runs FAST with ORB's fastThreshold): for each of the 16 arcs of 9 contiguous pixels
    of CIRCLE take the smallest signed difference, centre minus pixel (bright polarity) and pixel minus centre (dark); `best`
    is the largest of these over all arcs and both polarities.  A pixel is a corner iff best > t, and then scores best - 1
    (cornerScore<16>), else 0.  Only [3, w - 3) x [3, h - 3) is scanned; the border scores 0.  Exact integers."""
    I = np.asarray(img, np.int16)
    h, w = I.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    for y0 in range(3, h - 3, 256):                           # row bands: 16 difference planes of a 4K level fit in memory
        y1 = min(y0 + 256, h - 3)
        c = I[y0:y1, 3:w - 3]
        d = np.stack([c - I[y0 + dy:y1 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
        d = np.concatenate([d, d[:8]])                        # 24 planes: every arc of 9 is contiguous
        best = np.zeros(c.shape, np.int16)
        for sgn in (1, -1):
            e = sgn * d
            m2 = np.minimum(e[:-1], e[1:])                    # runs of 2, 4, 8, then 9
            m4 = np.minimum(m2[:-2], m2[2:])
            m8 = np.minimum(m4[:-4], m4[4:])
            m9 = np.minimum(m8[:16], e[8:24])
            best = np.maximum(best, m9.max(0))
        out[y0:y1, 3:w - 3] = np.where(best > t, best - 1, 0)
    return out


def fast_nms(score):
    """FAST's non-maximum suppression: a corner survives iff its score is strictly greater than each of its 8 neighbours
    (non-corners score 0; outside the image counts as 0).  -> bool mask."""
    s = np.asarray(score, np.int64)
    h, w = s.shape
    p = np.pad(s, 1)
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= s > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep


def umax(half):
    """The half-widths of ORB's circular patch (orb.cpp detectAndCompute): umax[v] = cvRound(sqrt(half^2 - v^2)) for
    v <= vmax = floor(half sqrt(2) / 2 + 1), then the rows above vmin = ceil(half sqrt(2) / 2) filled from the columns so that
    the disc is symmetric under x <-> y.  half + 2 entries, as OpenCV allocates."""
    r = float(np.float32(half) * np.sqrt(np.float32(2)) / np.float32(2))
    vmax, vmin = int(np.floor(r + 1)), int(np.ceil(r))
    u = np.zeros(half + 2, np.int64)
    for v in range(vmax + 1):
        u[v] = int(np.rint(np.sqrt(float(half * half - v * v))))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u


def disc_offsets(half):
    """(du, dv) of every pixel of the disc umax describes."""
    u = umax(half)
    du, dv = [], []
    for v in range(-half, half + 1):
        r = int(u[abs(v)])
        du.extend(range(-r, r + 1))
        dv.extend([v] * (2 * r + 1))
    return np.array(du, np.int64), np.array(dv, np.int64)


def ic_angle(level, x, y, half):
    """Intensity-centroid orientation (orb.cpp ICAngles), on the UNBLURRED level: m10 = sum u I(x + u, y + v) and
    m01 = sum v I(x + u, y + v) over the disc, angle = degrees(atan2(m01, m10)) mod 360, float64.  x, y: integer level
    coordinates (arrays)."""
    du, dv = disc_offsets(half)
    x = np.asarray(x, np.int64)[:, None]
    y = np.asarray(y, np.int64)[:, None]
    I = np.asarray(level, np.float64)[y + dv[None, :], x + du[None, :]]
    m10 = (I * du[None, :]).sum(1)
    m01 = (I * dv[None, :]).sum(1)
    return np.degrees(np.arctan2(m01, m10)) % 360.0


def brief(blurred, x, y, angle_deg, pattern):
    """Rotated BRIEF (orb.cpp computeOrbDescriptors), on the BLURRED level: each pattern point (px, py) is rotated by the
    keypoint's angle in float64, x' = px cos - py sin, y' = px sin + py cos, rounded half to even (cvRound) and sampled at
    (x + x', y + y'); bit b of byte j is I(p[16 j + 2 b]) < I(p[16 j + 2 b + 1]).  pattern: 1024 ints, (x, y) of 512 points.
    -> (bits bool [n, 256], ambiguous bool [n, 256]): a bit is ambiguous when one of its two samples has a rotated coordinate
    within BRIEF_MARGIN of a half-integer (the f32 rotation of an implementation may round it the other way)."""
    pts = np.asarray(pattern, np.float64).reshape(512, 2)
    a = np.radians(np.asarray(angle_deg, np.float64))[:, None]
    c, s = np.cos(a), np.sin(a)
    xr = pts[None, :, 0] * c - pts[None, :, 1] * s
    yr = pts[None, :, 0] * s + pts[None, :, 1] * c
    amb = (np.abs(xr - np.floor(xr) - 0.5) < BRIEF_MARGIN) | (np.abs(yr - np.floor(yr) - 0.5) < BRIEF_MARGIN)
    sx = np.asarray(x, np.int64)[:, None] + np.rint(xr).astype(np.int64)
    sy = np.asarray(y, np.int64)[:, None] + np.rint(yr).astype(np.int64)
    I = np.asarray(blurred)[sy, sx].astype(np.int64)
    bits = I[:, 0::2] < I[:, 1::2]
    return bits, amb[:, 0::2] | amb[:, 1::2]


def unpack_descriptors(desc):
    """[n, 32] bytes -> bool [n, 256] in brief()'s bit order (bit b of byte j at 8 j + b)."""
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little").astype(bool)


def area_taps(s, d):
    """One axis of resize(INTER_AREA) shrinking s -> d (image_utils.rs:17): destination cell i covers [i s / d, (i + 1) s / d)
    clipped to [0, s); source pixel k weighs |[k, k + 1) & cell| / |cell|, fractional edge cells included.
    -> (idx [d, K], weight [d, K], dropped [d]): `dropped` is the weight of the edge cells whose overlap is at most
    AREA_CUTOFF, which computeResizeAreaTab leaves out."""
    scale = s / d
    a = np.arange(d) * scale
    b = np.minimum(a + scale, s)
    K = int(np.ceil(scale)) + 1
    idx = np.floor(a).astype(np.int64)[:, None] + np.arange(K)[None, :]
    ov = np.clip(np.minimum(b[:, None], idx + 1) - np.maximum(a[:, None], idx), 0.0, None)
    w = ov / (b - a)[:, None]
    small = (ov > 0) & (ov <= AREA_CUTOFF * (1 + 1e-6))
    return np.clip(idx, 0, s - 1), w, (w * small).sum(1)


def area_resize(img, dw, dh):
    """resize(INTER_AREA) (image_utils.rs:8-20 to_small_image): every destination pixel is the exact overlap-weighted mean of
    its source box, fractional edge cells included, float64, unrounded.  -> (mean [dh, dw(, c)], (iy, wy), (ix, wx)): the
    separable source weights, destination (i, j) weighs source (iy[i, a], ix[j, b]) by wy[i, a] wx[j, b]."""
    f = np.asarray(img, np.float64)
    iy, wy, _ = area_taps(f.shape[0], dh)
    ix, wx, _ = area_taps(f.shape[1], dw)
    ey = (slice(None), None) + (None,) * (f.ndim - 2)        # weights broadcast over the other axes
    ex = (None, slice(None)) + (None,) * (f.ndim - 2)
    r = sum(f[iy[:, k]] * wy[:, k][ey] for k in range(iy.shape[1]))
    return sum(r[:, ix[:, k]] * wx[:, k][ex] for k in range(ix.shape[1])), (iy, wy), (ix, wx)


def area_eta(sw, sh, dw, dh):
    """How far a correct f32 INTER_AREA (OpenCV's computeResizeAreaTab + ResizeArea_Invoker, the restatement's ocv.area 0) may lie
    from area_resize, per destination pixel [dh, dw], in grey levels.  Derivation:
      * the 1e-3 cut-off leaves out edge cells whose overlap is at most 1e-3; their weight (area_taps' `dropped`) is lost, so the
        sum moves by at most 255 (dropped_y + dropped_x) (a union bound on the 2-D weight lost);
      * the weights are f32 (relative error u = 2^-24 each), the row sums of Kx products and the column sum of Ky products are
        f32: a recursive sum of n products with rounded weights errs by at most gamma_(n+2) times the sum of |terms| <= 255
        (gamma_n = n u / (1 - n u)); the two sums nest, so n = Kx + Ky + 2 covers it (the integer-factor fast path multiplies
        an exact integer sum by the f32 1 / area: one rounding less);
      * the double cell boundaries of the table differ from the exact s / d by about 1e-13, far below the f32 terms.
    eta < 0.5 holds for every shape this project runs, so a mean farther than eta from a rounding boundary rounds to the same
    integer, and every output is within 0.5 + eta < 1 of the mean."""
    _, wy, dy = area_taps(sh, dh)
    _, wx, dx = area_taps(sw, dw)
    n = wy.shape[1] + wx.shape[1] + 2
    gamma = n * F32_U / (1 - n * F32_U)
    return 255.0 * (dy[:, None] + dx[None, :]) + 255.0 * gamma + 1e-9


def small_size(w, h, area=120000):
    """image_utils.rs:8-16: factor = sqrt(area as f32 / (w h) as f32) in f32, each side (side as f32 * factor) as i32
    (truncation)."""
    f32 = np.float32
    factor = np.sqrt(f32(area) / f32(w * h))
    return int(f32(w) * factor), int(f32(h) * factor)


def _map(M, dw, dh):
    """-> (X, Y, W == 0, margin): the source position of every destination pixel and the rounding margin of the map's kind
    (a 2x3 matrix or a 3x3 one with third row (0, 0, 1) is warpAffine's)."""
    M = np.asarray(M, np.float64).reshape(-1)
    if M.size == 6:
        M = np.concatenate([M, [0.0, 0.0, 1.0]])
    affine = M[6] == 0 and M[7] == 0 and M[8] == 1
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    W = M[6] * x + M[7] * y + M[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        X = (M[0] * x + M[1] * y + M[2]) / W
        Y = (M[3] * x + M[4] * y + M[5]) / W
    return X, Y, W == 0, WARP_MARGIN if affine else PERSP_MARGIN


def _near_half(v, margin):
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.floor(v) - 0.5) <= margin


def warp_nearest(src, M, dw, dh):
    """warpAffine / warpPerspective(src, M, (dw, dh), INTER_NEAREST | WARP_INVERSE_MAP, BORDER_CONSTANT 0) (lib.rs:339-347):
    destination pixel (x, y) maps through M (2x3, or 3x3 with the division by the third row) to a source position in float64
    and takes the nearest source pixel, 0 outside the frame.  -> (out [dh, dw, c], ambiguous bool [dh, dw]): a pixel is
    ambiguous when a mapped coordinate lies within WARP_MARGIN of a half-integer for an affine map (OpenCV's 10-bit fixed
    point may round it either way), within PERSP_MARGIN for a projective one, or its projective denominator is 0."""
    src = np.asarray(src)
    X, Y, zero, margin = _map(M, dw, dh)
    big = ~(np.abs(X) < 1e7) | ~(np.abs(Y) < 1e7)             # also NaN: far outside any frame (OpenCV saturates)
    xi = np.where(big, -1, np.floor(np.where(big, 0, X) + 0.5)).astype(np.int64)
    yi = np.where(big, -1, np.floor(np.where(big, 0, Y) + 0.5)).astype(np.int64)
    inside = (xi >= 0) & (xi < src.shape[1]) & (yi >= 0) & (yi < src.shape[0])
    out = np.zeros((dh, dw) + src.shape[2:], src.dtype)
    out[inside] = src[yi[inside], xi[inside]]
    amb = zero | (~big & (_near_half(X, margin) | _near_half(Y, margin)))
    return out, amb


def warp_spread(src, M, dw, dh):
    """Per destination pixel and channel, how far any pixel a correct nearest warp may pick lies from warp_nearest's: the
    range (max - min) over the 1, 2 or 4 source pixels (0 outside the frame) that the ambiguous coordinates round to; 0 where
    the pixel is not ambiguous, 255 where the denominator is 0."""
    src = np.asarray(src)
    X, Y, zero, margin = _map(M, dw, dh)
    big = ~(np.abs(X) < 1e7) | ~(np.abs(Y) < 1e7)
    X = np.where(big, -10.0, X); Y = np.where(big, -10.0, Y)
    ax, ay = _near_half(X, margin), _near_half(Y, margin)
    nx, ny = np.floor(X + 0.5).astype(np.int64), np.floor(Y + 0.5).astype(np.int64)
    cands = []
    for ox in (0, 1):
        for oy in (0, 1):
            cx = np.where(ax, np.floor(X).astype(np.int64) + ox, nx)
            cy = np.where(ay, np.floor(Y).astype(np.int64) + oy, ny)
            ok = (cx >= 0) & (cx < src.shape[1]) & (cy >= 0) & (cy < src.shape[0])
            v = np.zeros((dh, dw) + src.shape[2:], np.int64)
            v[ok] = src[cy[ok], cx[ok]]
            cands.append(v)
    c = np.stack(cands)
    spread = (c.max(0) - c.min(0)).astype(np.float64)
    spread[zero] = 255.0
    return spread


def similarity(a, b):
    """compute_similarity (image_utils.rs:22-27): 1 - ||a - b||_2 / sqrt(255^2 * 3 * p), p = pixels, float64."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    p = a.shape[0] * a.shape[1]
    return 1.0 - np.sqrt(((a - b) ** 2).sum()) / np.sqrt(255.0 ** 2 * 3 * p)


def reprojection(frame, M, page_w, page_h, small_area=120000):
    """The re-projection of lib.rs:335-351 in float64: the frame warped to the page's size (warp_nearest), then the exact
    INTER_AREA mean of that to the page's small size.  -> (mean [sh, sw, 3], delta [sh, sw, 3]): delta is how many grey levels
    a correct implementation's rounded small image may lie from rint(mean) (see similarity_bound)."""
    sw, sh = small_size(page_w, page_h, small_area)
    warped, _ = warp_nearest(frame, M, page_w, page_h)
    mean, _, _ = area_resize(warped, sw, sh)
    spread, _, _ = area_resize(warp_spread(frame, M, page_w, page_h), sw, sh)
    reach = spread + area_eta(page_w, page_h, sw, sh)[:, :, None]
    r = np.rint(mean)
    delta = np.maximum(np.abs(np.rint(mean + reach) - r), np.abs(np.rint(mean - reach) - r))
    return mean, delta


def reprojection_similarity(frame, M, page_w, page_h, page_small, rep=None):
    """The similarity of lib.rs:348-350 by definition: similarity(rint(re-projected mean), page_small).  rep: reprojection()'s
    result for these arguments (computed when None)."""
    mean, _ = rep if rep is not None else reprojection(frame, M, page_w, page_h)
    return similarity(np.rint(mean), page_small)


def similarity_bound(frame, M, page_w, page_h, page_small, rep=None):
    """How far a correct implementation's similarity may lie from reprojection_similarity.  A correct small image differs from
    a = rint(mean) by at most delta per channel:
      * its f32 INTER_AREA sum lies within eta (area_eta) of the mean of ITS warped image;
      * its warped image equals warp_nearest's except at ambiguous pixels, where it holds one of the pixels the ambiguous
        coordinates may round to: the box mean moves by at most sum(weight * warp_spread) over the box (the actual spread of the
        candidates in place of 255, never larger);
      * so its sum lies within D = that + eta of the mean, and delta = the largest |rint(v) - rint(mean)| over |v - mean| <= D:
        1 when the mean is within eta of a rounding boundary, 0 when it is not and nothing in its box is ambiguous.
    Over the box a' in [a - delta, a + delta], ||a' - b||_2 (b = page_small) is largest at sqrt(sum (|a - b| + delta)^2) and
    smallest at sqrt(sum max(|a - b| - delta, 0)^2), channel by channel; the bound is the larger distance of these from
    ||a - b||_2, over max_error.  (It never exceeds ||delta||_2 / max_error, the 1-Lipschitz bound of the L2 norm.)  Plus 1e-6
    for the f32 quotient and subtraction of compute_similarity."""
    mean, delta = rep if rep is not None else reprojection(frame, M, page_w, page_h)
    r = np.abs(np.rint(mean) - np.asarray(page_small, np.float64))
    n0 = np.sqrt((r * r).sum())
    hi = np.sqrt(((r + delta) ** 2).sum())
    lo = np.sqrt((np.maximum(r - delta, 0.0) ** 2).sum())
    return max(hi - n0, n0 - lo) / np.sqrt(255.0 ** 2 * 3 * delta.shape[0] * delta.shape[1]) + 1e-6
