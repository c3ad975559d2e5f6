"""Test-side float64 definitions of the SIFT steps (Lowe, "Distinctive Image Features from Scale-Invariant Keypoints", IJCV 2004,
sections 3-6, with the conventions OpenCV documents for cv::SIFT: the doubled first octave, nOctaveLayers = 3, 36 orientation
bins, the 4 x 4 x 8 descriptor scaled by 512), written from the paper and those conventions, not from oracle/ or the kernels.

Plain numpy, float64 or exact integers.  Nothing here imports the restatement or the product.  tests/f64_checks.py holds an
implementation's own upstream outputs to these definitions step by step; tests/test_oracle_sift_definitions.py runs that on
the CPU restatement and tests/test_gpu_sift_definitions.py on the HIP kernels."""
import numpy as np

NL = 3                 # nOctaveLayers
BINS = 36              # orientation histogram bins
BORDER = 5             # extrema stay this far inside a layer
MAX_STEPS = 5          # Newton steps of the sub-pixel refinement
ORI_RADIUS = 4.5       # orientation window radius, in units of the keypoint's scale
ORI_SIGMA = 1.5        # orientation weight sigma, same units
PEAK_RATIO = 0.8       # secondary orientation peaks reach this share of the largest
D_CELLS, D_BINS = 4, 8             # descriptor: 4 x 4 cells of 8 orientation bins
D_WIDTH = 3.0          # cell width, in units of the keypoint's scale
D_CLAMP = 0.2          # descriptor values are clamped at this share of the norm
D_SCALE = 512.0        # and the clamped vector is scaled to this norm


def cv_round(x):
    """cvRound: nearest integer, ties to even."""
    return int(np.rint(x))


# ---- images ----------------------------------------------------------------------------------------------------------------

def reflect101(i, n):
    """BORDER_REFLECT_101 index (dcb|abcd|cba), reflected as often as it takes when |i| exceeds the side."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def num_taps(s):
    """Taps of a Gaussian blur of sigma s: cvRound(8 s + 1) | 1."""
    return cv_round(8.0 * s + 1.0) | 1


def gauss_taps(s):
    n = num_taps(s)
    x = np.arange(n) - (n - 1) / 2
    k = np.exp(-x * x / (2.0 * s * s))
    return k / k.sum()


def blur(img, s):
    """Separable Gaussian blur of sigma s, BORDER_REFLECT_101, in float64."""
    a = np.asarray(img, np.float64)
    k = gauss_taps(s)
    n, r = len(k), len(k) // 2
    h, w = a.shape
    t = a[:, reflect101(np.arange(-r, w + r), w)]
    t = sum(k[j] * t[:, j:j + w] for j in range(n))
    t = t[reflect101(np.arange(-r, h + r), h)]
    return sum(k[j] * t[j:j + h] for j in range(n))


def upsample2(g):
    """2x bilinear upsample: destination pixel d sits at (d + 0.5) / 2 - 0.5 of the source, neighbours clamped to the image."""
    g = np.asarray(g, np.float64)

    def axis(n):
        f = (np.arange(2 * n) + 0.5) * 0.5 - 0.5
        i0 = np.floor(f)
        a = f - i0
        i0 = i0.astype(np.int64)
        return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), a

    y0, y1, ay = axis(g.shape[0])
    x0, x1, ax = axis(g.shape[1])
    t = g[:, x0] * (1 - ax) + g[:, x1] * ax
    return t[y0] * (1 - ay)[:, None] + t[y1] * ay[:, None]


def base_sigma(sigma):
    """The doubled image is taken to carry a blur of 2 * 0.5 already: sig_diff = sqrt(max(sigma^2 - 1, 0.01))."""
    return float(np.sqrt(max(sigma * sigma - 1.0, 0.01)))


def base_image(gray, sigma):
    """Layer 0 of octave 0 from the gray image."""
    return blur(upsample2(gray), base_sigma(sigma))


def layer_sigmas(sigma, nl=NL):
    """The blur that takes layer i - 1 to layer i (i = 1 .. nl + 2): sigma k^(i-1) sqrt(k^2 - 1), k = 2^(1/nl)."""
    k = 2.0 ** (1.0 / nl)
    return [sigma * k ** (i - 1) * np.sqrt(k * k - 1.0) for i in range(1, nl + 3)]


def octave_sizes(w, h, nl=NL):
    """(height, width) of every octave for a w x h input: cvRound(log2(min side of the doubled image) - 2) + 1 octaves, each
    every second pixel of the one before (floor sizes)."""
    n = max(cv_round(np.log2(min(2 * w, 2 * h)) - 2.0) + 1, 0)
    out, ow, oh = [], 2 * w, 2 * h
    for _ in range(n):
        out.append((oh, ow))
        ow, oh = ow // 2, oh // 2
    return out


def blur_plan(w, h, sigma, nl=NL):
    """Every Gaussian blur of the pyramid of a w x h input: [(octave, layer, taps, layer width, layer height)]."""
    sizes = octave_sizes(w, h, nl)
    plan = [(0, 0, num_taps(base_sigma(sigma)), sizes[0][1], sizes[0][0])] if sizes else []
    for o, (oh, ow) in enumerate(sizes):
        plan += [(o, i + 1, num_taps(s), ow, oh) for i, s in enumerate(layer_sigmas(sigma, nl))]
    return plan


# ---- extrema and their refinement ------------------------------------------------------------------------------------------

def raw_extrema(prev, cur, nxt, ct=0.04, nl=NL):
    """(rows, cols) of the scale-space extrema of DoG layer `cur`: |v| > floor(0.5 ct / nl 255), v >= (v > 0) or <= (v <= 0)
    all 26 neighbours, at least BORDER pixels inside.  Row-major order."""
    thr = np.floor(0.5 * ct / nl * 255.0)
    h, w = cur.shape
    b = BORDER
    if h <= 2 * b or w <= 2 * b:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    S = np.stack([prev, cur, nxt])
    nb = np.stack([S[:, b + dy:h - b + dy, b + dx:w - b + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    v = cur[b:h - b, b:w - b]
    ext = (np.abs(v) > thr) & (((v > 0) & (v >= nb.max(axis=(0, 1)))) | ((v <= 0) & (v <= nb.min(axis=(0, 1)))))
    r, c = np.nonzero(ext)
    return r + b, c + b


def _quadratic(cube, dtype):
    """Gradient (x, y, s) and Hessian of the 3 x 3 x 3 DoG neighbourhood cube[s, y, x], central differences of pixel values
    scaled by 1/255: first derivatives x 1/2, second x 1, mixed x 1/4."""
    f = dtype
    q = cube.astype(f)
    s = f(1) / f(255)
    v = q[1, 1, 1]
    lo = np.array([q[1, 1, 0], q[1, 0, 1], q[0, 1, 1]], f)
    hi = np.array([q[1, 1, 2], q[1, 2, 1], q[2, 1, 1]], f)
    g = (hi - lo) * (s * f(0.5))
    diag = (hi + lo - f(2) * v) * s
    dxy = (q[1, 2, 2] - q[1, 2, 0] - q[1, 0, 2] + q[1, 0, 0]) * (s * f(0.25))
    dxs = (q[2, 1, 2] - q[2, 1, 0] - q[0, 1, 2] + q[0, 1, 0]) * (s * f(0.25))
    dys = (q[2, 2, 1] - q[2, 0, 1] - q[0, 2, 1] + q[0, 0, 1]) * (s * f(0.25))
    H = np.array([[diag[0], dxy, dxs], [dxy, diag[1], dys], [dxs, dys, diag[2]]], f)
    return v * s, g, H


def _solve_sym3(H, g):
    """H^-1 g of a symmetric 3 x 3 H through the cross products of its rows (the adjugate); 0 where H is singular."""
    c12, c20, c01 = np.cross(H[1], H[2]), np.cross(H[2], H[0]), np.cross(H[0], H[1])
    det = H[0] @ c12
    if det == 0:
        return np.zeros(3, H.dtype)
    return np.array([g @ c12, g @ c20, g @ c01], H.dtype) / det


def refine(D, layer, r, c, octave, sigma, ct=0.04, et=10.0, nl=NL, dtype=np.float64):
    """Sub-pixel refinement of the extremum (layer, r, c) of one octave's DoG layers D[0 .. nl + 1] (Lowe section 4): at most
    MAX_STEPS Newton steps on the 3-D quadratic; a step whose offsets are all below 0.5 ends the walk, any other moves the
    sample point by the rounded offsets and the point must stay inside (layers 1 .. nl, BORDER pixels); then the contrast test
    |D^| nl >= ct and the edge test tr^2 e < (e + 1)^2 det with det > 0.

    -> None when the walk leaves the octave or does not end, else a dict: accepted, layer, r, c, the offsets off = (xc, xr, xi),
    x, y, size (input-image scale: the doubled image's halved), response, xi_byte = cvRound((xi + 0.5) 255), octave_field
    (octave - 1 as a byte | layer << 8 | xi_byte << 16) and margin: the smallest distance of any decision on the way from its
    boundary — offsets from 0.5 (and from a rounding tie where the point moves) in pixels, the contrast and edge tests relative.
    dtype = np.float32 evaluates the same formulas in f32 (f64_checks measures the f32 error of the solve with it)."""
    f = dtype
    h, w = D[0].shape
    margin = np.inf
    for _ in range(MAX_STEPS):
        cube = np.stack([D[layer + k][r - 1:r + 2, c - 1:c + 2] for k in (-1, 0, 1)])
        v, g, H = _quadratic(cube, f)
        off = -_solve_sym3(H, g)
        a = np.abs(off).astype(np.float64)
        margin = min(margin, np.abs(a - 0.5).min())
        if (a < 0.5).all():
            break
        if (a > 2.0 ** 31 / 3).any():
            return None
        margin = min(margin, np.abs(a - np.floor(a) - 0.5).min())
        c += cv_round(off[0]); r += cv_round(off[1]); layer += cv_round(off[2])
        if layer < 1 or layer > nl or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return None
    else:
        return None
    contr = v + f(0.5) * (g @ off)
    resp = abs(float(contr))
    m_contrast = abs(resp * nl - ct) / ct
    tr = H[0, 0] + H[1, 1]
    det = H[0, 0] * H[1, 1] - H[0, 1] * H[0, 1]
    lhs, rhs = float(tr * tr) * et, (et + 1.0) ** 2 * float(det)
    m_edge = abs(lhs - rhs) / max(abs(lhs) + abs(rhs), 1e-300)
    accepted = resp * nl >= ct and det > 0 and lhs < rhs
    xi = float(off[2])
    xi_byte = cv_round((xi + 0.5) * 255.0)
    scale = 2.0 ** octave * 0.5
    return dict(accepted=bool(accepted), margin=float(min(margin, m_contrast, m_edge)), layer=layer, r=r, c=c,
                off=np.asarray(off, np.float64), x=(c + float(off[0])) * scale, y=(r + float(off[1])) * scale,
                size=sigma * 2.0 ** ((layer + xi) / nl) * 2.0 * scale, response=resp, xi_byte=xi_byte,
                octave_field=((octave - 1) & 255) | (layer << 8) | (xi_byte << 16),
                resp_terms=float(abs(v) + np.abs(g * off).sum()), grad_l1=float(np.abs(g).sum()))


# ---- orientation -----------------------------------------------------------------------------------------------------------

def _gradients(L, y, x):
    dx = L[y, x + 1] - L[y, x - 1]
    dy = L[y - 1, x] - L[y + 1, x]                              # image rows grow downwards: angles are counter-clockwise
    return dx, dy


SMOOTH = np.array([1, 4, 6, 4, 1]) / 16.0


def smooth_circular(raw):
    n = len(raw)
    return sum(SMOOTH[k] * np.roll(raw, 2 - k) for k in range(5)) if n else raw


def orientation_hist(L, r, c, scl, atan_err=0.0, quantum=0.0):
    """Smoothed 36-bin gradient orientation histogram around (r, c) of Gaussian layer L (Lowe section 5): window radius
    cvRound(4.5 scl), weights exp(-d^2 / 2 (1.5 scl)^2), exact atan2, bin = round(angle / 10) mod 36, 1-4-6-4-1 circular
    smoothing.  -> (hist, slack): slack[k] bounds how far hist[k] moves when every sample's angle is off by at most atan_err
    degrees (the mass within atan_err of the boundary between two bins may sit in either; smoothing weighs a bin and its
    neighbour at most 3/16 apart) and every sample's contribution by at most quantum (an implementation that sums in fixed
    point)."""
    h, w = L.shape
    radius = cv_round(ORI_RADIUS * scl)
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = r + ii, c + jj
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, ii, jj = y[ok], x[ok], ii[ok], jj[ok]
    dx, dy = _gradients(L, y, x)
    sg = ORI_SIGMA * scl
    m = np.exp(-(ii * ii + jj * jj) / (2.0 * sg * sg)) * np.hypot(dx, dy)
    t = (np.degrees(np.arctan2(dy, dx)) % 360.0) * (BINS / 360.0)
    b = np.floor(t + 0.5).astype(np.int64)
    raw = np.bincount(b % BINS, m, BINS)
    hist = smooth_circular(raw)
    slack = smooth_circular(np.bincount(b % BINS, None, BINS) * quantum)
    if atan_err > 0:
        e = atan_err * BINS / 360.0
        fr = t + 0.5 - np.floor(t + 0.5)                        # 0 at the boundary below bin b, 1 at the one above
        up = np.bincount(b % BINS, m * (fr > 1 - e), BINS)      # mass that may sit in bin b + 1 instead
        dn = np.bincount((b - 1) % BINS, m * (fr < e), BINS)    # mass that may sit in bin b - 1: boundary (b - 1 | b)
        edge = up + dn                                          # edge[j]: undecided between bins j and j + 1
        dw = np.abs(np.diff(np.r_[0.0, SMOOTH, 0.0]))           # |w(k - j) - w(k - j - 1)|, k - j = -2 .. 3
        slack = slack + sum(dw[i] * np.roll(edge, i - 2) for i in range(6))
    return hist, slack


def orientation_peaks(hist, margin=0.0):
    """Peaks of the smoothed histogram: above both neighbours and >= 0.8 max; parabolic interpolation of the bin;
    angle = 360 - 10 bin (mod 360).  -> [(angle, bin j, m)], m = min(hist[j] - larger neighbour, hist[j] - 0.8 max) / max: a
    peak by definition has m > 0 (>= 0 for the ratio); bins with m > -margin are listed as well, so that a caller can tell a
    decided peak (m > margin) from an undecided one (|m| <= margin)."""
    n = len(hist)
    mx = hist.max()
    out = []
    if mx <= 0:
        return out
    for j in range(n):
        l, c, r = hist[(j - 1) % n], hist[j], hist[(j + 1) % n]
        m = min(c - max(l, r), c - PEAK_RATIO * mx) / mx
        den = l - 2 * c + r
        if m > -margin and den != 0:
            b = (j + 0.5 * (l - r) / den) % n
            out.append(((360.0 - 360.0 / n * b) % 360.0, j, float(m)))
    return out


# ---- selection -------------------------------------------------------------------------------------------------------------

def retain_best(response, n):
    """Mask of the keypoints kept for nfeatures = n: every response that reaches the n-th largest (ties kept); all for n <= 0
    or no more than n keypoints."""
    response = np.asarray(response)
    if n <= 0 or len(response) <= n:
        return np.ones(len(response), bool)
    return response >= np.sort(response)[::-1][n - 1]


def canonical_keys(octave, layer, r, c, peak_bin):
    """Sort key of the canonical keypoint order: (octave, layer, row, column, peak bin) ascending."""
    return [tuple(int(v) for v in t) for t in zip(octave, layer, r, c, peak_bin)]


# ---- descriptor ------------------------------------------------------------------------------------------------------------

def descriptor(L, x, y, ori, scl, detail=False, atan_err=0.0):
    """The 128 unrounded descriptor values of a keypoint at (x, y) of Gaussian layer L with orientation ori (degrees, counter-
    clockwise) and scale scl (Lowe section 6): samples within radius cvRound(3 scl sqrt(2) 2.5) (at most the image diagonal) of
    the rounded position, rotated into the keypoint's frame and scaled to cells of width 3 scl; each sample's gradient magnitude,
    weighted by exp(-(r^2 + c^2) / 8) of its cell coordinates, is shared trilinearly between the neighbouring cells (4 x 4;
    votes beyond the grid are dropped) and orientation bins (8, circular; relative to ori); the vector is clamped at 0.2 of its
    norm and scaled to norm 512.

    detail: also a dict for error bounds — raw (the 128 sums before the clamp), support (per element: the spatially weighted
    magnitude of every sample whose orientation, known to atan_err degrees, lies within one bin of the element's: the
    orientation weight is a hat function of slope 1 per bin, so an error of e bins moves at most e x support into or out of
    the element), votes (samples voting per element), norm, clamped_norm."""
    d, n = D_CELLS, D_BINS
    h, w = L.shape
    px, py = cv_round(x), cv_round(y)
    hw = D_WIDTH * scl
    radius = min(cv_round(hw * np.sqrt(2.0) * (d + 1) * 0.5), int(np.sqrt(float(w) * w + float(h) * h)))
    ct, st = np.cos(np.radians(ori)) / hw, np.sin(np.radians(ori)) / hw
    ii, jj = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    cr, rr = jj * ct - ii * st, jj * st + ii * ct
    rb, cb = rr + d / 2 - 0.5, cr + d / 2 - 0.5
    r, c = py + ii, px + jj
    ok = (rb > -1) & (rb < d) & (cb > -1) & (cb < d) & (r > 0) & (r < h - 1) & (c > 0) & (c < w - 1)
    rb, cb, r, c, cr, rr = rb[ok], cb[ok], r[ok], c[ok], cr[ok], rr[ok]
    dx, dy = _gradients(L, r, c)
    mag = np.hypot(dx, dy) * np.exp(-(cr * cr + rr * rr) / (d * d * 0.5))
    ob = ((np.degrees(np.arctan2(dy, dx)) % 360.0) - ori) * (n / 360.0)
    r0, c0, o0 = np.floor(rb).astype(np.int64), np.floor(cb).astype(np.int64), np.floor(ob).astype(np.int64)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    size = (d + 2) * (d + 2) * n
    H, S, V = np.zeros(size), np.zeros(size), np.zeros(size)
    for a, wa in ((0, 1 - fr), (1, fr)):
        for b, wb in ((0, 1 - fc), (1, fc)):
            cell = ((r0 + 1 + a) * (d + 2) + (c0 + 1 + b)) * n
            for e, we in ((0, 1 - fo), (1, fo)):
                H += np.bincount(cell + (o0 + e) % n, mag * wa * wb * we, size)
                V += np.bincount(cell + (o0 + e) % n, None, size)
            if detail:
                eps = atan_err * n / 360.0                      # the two bins the sample votes for, and a third when the
                for e, on in ((-1, fo < eps), (0, True), (1, True), (2, fo > 1 - eps)):     # error can carry it past a bin centre
                    S += np.bincount(cell + (o0 + e) % n, mag * wa * wb * on, size)
    pick = lambda A: A.reshape(d + 2, d + 2, n)[1:d + 1, 1:d + 1].reshape(-1)
    raw = pick(H)
    nrm = np.linalg.norm(raw)
    v = np.minimum(raw, D_CLAMP * nrm)
    cn = max(np.linalg.norm(v), 2.0 ** -23)
    v = v * (D_SCALE / cn)
    if detail:
        return v, dict(raw=raw, support=pick(S), votes=pick(V), norm=nrm, clamped_norm=cn)
    return v
