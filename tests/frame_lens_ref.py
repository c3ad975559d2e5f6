"""The frame lens (include/slideo_amd.h "Frame lens") and the placement lens ("Placement lens") restated in numpy, written from the
header: float64, every operation one numpy operation (rounded on its own, nothing fused), a whole image at once.  `undistort` is the
definition the HIP kernels (csrc/frame_lens.hip.h) are held to bit for bit; `exact_coords` is the float64 ideal behind the derived
bound of tests/test_gpu_frame_lens.py; `placement_lens` is the learner with numpy.linalg in place of the library's own solvers.
Taps and blend are tests/frame_region_ref.py's.  Nothing here calls the library."""
import numpy as np

import frame_region_ref as R
import placement_ref as P

INT_MIN, INT_MAX = R.INT_MIN, R.INT_MAX


def defaults(src_w, src_h):
    """The mirrors' defaults: the image centre and half the source diagonal."""
    return (src_w - 1) / 2.0, (src_h - 1) / 2.0, 0.5 * float(np.hypot(src_w, src_h))


def point(cx, cy, f, k1, k2, u, v):
    """Step 2: where the camera sees the ideal point(s) (u, v)."""
    cx, cy, f, k1, k2 = (np.float64(a) for a in (cx, cy, f, k1, k2))
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    q = np.float64(1.0) / (f * f)
    with np.errstate(all="ignore"):
        dx, dy = u - cx, v - cy
        r2 = (dx * dx + dy * dy) * q
        t = r2 * k2
        t = k1 + t
        t = r2 * t
        g = 1.0 + t
        return cx + dx * g, cy + dy * g


def ideal(M, out_w, out_h):
    """Step 1: the ideal point (u, v) of every destination pixel, float64 [out_h, out_w] each.  M None: no region."""
    x = np.arange(out_w, dtype=np.float64)[None, :]
    y = np.arange(out_h, dtype=np.float64)[:, None]
    if M is None:
        return x + 0.0 * y, y + 0.0 * x
    M = np.asarray(M, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        N0 = (M[0] * x + M[1] * y) + M[2]
        N1 = (M[3] * x + M[4] * y) + M[5]
        W = (M[6] * x + M[7] * y) + M[8]
        Wi = 1.0 / W
        return N0 * Wi, N1 * Wi


def _round_sat(v):
    """rect_round_sat: v < hi ? v : hi, then > lo ? v : lo (a NaN becomes INT_MAX), then rint."""
    v = np.where(v < INT_MAX, v, INT_MAX)
    v = np.where(v > INT_MIN, v, INT_MIN)
    return np.rint(v).astype(np.int64)


def coords(lens, M, out_w, out_h):
    """Steps 1 to 3: X, Y (int64 [out_h, out_w], 1/32 steps).  lens = (cx, cy, f, k1, k2)."""
    u, v = ideal(M, out_w, out_h)
    xd, yd = point(*lens, u, v)
    with np.errstate(all="ignore"):
        return _round_sat(32.0 * xd), _round_sat(32.0 * yd)


def undistort(img, lens, M=None, out_w=None, out_h=None):
    """img uint8 [h, w, 3] -> the analysed image uint8 [out_h, out_w, 3] (the source's size without a region)."""
    img = np.asarray(img, np.uint8)
    h, w, _ = img.shape
    if M is None:
        out_w, out_h = w, h
    X, Y = coords(lens, M, out_w, out_h)
    sx, ax, sy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    I = img.astype(np.int64)
    ax, ay = ax[:, :, None], ay[:, :, None]
    acc = I[y0, x0] * ((32 - ax) * (32 - ay)) + I[y0, x1] * (ax * (32 - ay)) + I[y1, x0] * ((32 - ax) * ay) + I[y1, x1] * (ax * ay)
    return ((acc + 512) >> 10).astype(np.uint8)


def exact_coords(lens, M, out_w, out_h):
    """The float64, unquantised source coordinate of every destination pixel."""
    u, v = ideal(M, out_w, out_h)
    return point(*lens, u, v)


def bend(frames, lens):
    """What a camera with the lens sees of the ideal frames uint8 [n, h, w, 3]: camera pixel D(p) shows the ideal frame at p.  The
    radius is inverted by Newton's method (60 steps, to machine precision) and the ideal frame is sampled bilinearly in float64 under
    the replicate border.  Written from the forward model alone: nothing of the code under test."""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    cx, cy, f, k1, k2 = lens
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rd = np.hypot(X - cx, Y - cy) / f
    r = rd.copy()
    for _ in range(60):
        r = r - (r * (1 + k1 * r * r + k2 * r ** 4) - rd) / (1 + 3 * k1 * r * r + 5 * k2 * r ** 4)
    g = 1 + k1 * r * r + k2 * r ** 4
    u, v = cx + (X - cx) / g, cy + (Y - cy) / g
    return np.stack([np.clip(np.rint(R.bilinear_f64(fr, u, v)), 0, 255).astype(np.uint8) for fr in frames])


# ---- the rules ---------------------------------------------------------------------------------------------------------------------

def monotone(k1, k2, R2):
    """1 + 3 k1 s + 5 k2 s^2 > 0 at 0, at R2 and at the vertex inside (0, R2)."""
    if not np.isfinite(R2) or R2 < 0:
        return False
    d = lambda s: 1.0 + 3.0 * k1 * s + 5.0 * k2 * s * s
    if not (d(0.0) > 0 and d(R2) > 0):
        return False
    if k2 != 0:
        sv = -3.0 * k1 / (10.0 * k2)
        if 0 < sv < R2 and not d(sv) > 0:
            return False
    return True


def reach(lens, src_w, src_h, M=None, out_w=None, out_h=None):
    """R2: the largest r2 of the ideal images of the four destination corners."""
    cx, cy, f = lens[:3]
    dw, dh = (src_w, src_h) if M is None else (out_w, out_h)
    r = []
    for y in (0.0, dh - 1.0):
        for x in (0.0, dw - 1.0):
            u, v = x, y
            if M is not None:
                m = np.asarray(M, np.float64).reshape(9)
                W = m[6] * x + m[7] * y + m[8]
                u, v = (m[0] * x + m[1] * y + m[2]) / W, (m[3] * x + m[4] * y + m[5]) / W
            r.append(((u - cx) ** 2 + (v - cy) ** 2) / (f * f))
    return max(r)


# ---- the learner ------------------------------------------------------------------------------------------------------------------
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, REL_STOP, PIVOT = 1e-3, 1e-12, 1e8, 1e-12, 1e-12


def _model(p, s, cx, cy, q, u, v, jac=False):
    """D(s H(u, v)) for parameters p = (h0 .. h7, k1[, k2]) -> (X, Y, r2[, J [2, N, len(p)]])."""
    h, k1, k2 = p[:8], p[8], (p[9] if len(p) == 10 else 0.0)
    with np.errstate(all="ignore"):
        w = h[6] * u + h[7] * v + 1.0
        Px, Py = s * ((h[0] * u + h[1] * v + h[2]) / w), s * ((h[3] * u + h[4] * v + h[5]) / w)
        a, b = Px - cx, Py - cy
        r2 = (a * a + b * b) * q
        g = 1.0 + r2 * (k1 + r2 * k2)
        X, Y = cx + a * g, cy + b * g
        if not jac:
            return X, Y, r2
        gp = k1 + 2.0 * k2 * r2
        xx, xy, yy = g + 2.0 * q * gp * a * a, 2.0 * q * gp * a * b, g + 2.0 * q * gp * b * b
        z = np.zeros_like(u)
        dPx = np.stack([s * u / w, s * v / w, s / w, z, z, z, -Px * u / w, -Px * v / w], 1)
        dPy = np.stack([z, z, z, s * u / w, s * v / w, s / w, -Py * u / w, -Py * v / w], 1)
        Jx = xx[:, None] * dPx + xy[:, None] * dPy
        Jy = xy[:, None] * dPx + yy[:, None] * dPy
        kx, ky = [a * r2], [b * r2]
        if len(p) == 10:
            kx.append(a * r2 * r2); ky.append(b * r2 * r2)
        return X, Y, r2, np.stack([np.concatenate([Jx, np.stack(kx, 1)], 1), np.concatenate([Jy, np.stack(ky, 1)], 1)])


def _cost(p, geo, u, v, X, Y):
    px, py, _ = _model(p, *geo, u, v)
    c = float(((px - X) ** 2 + (py - Y) ** 2).sum())
    return c if np.isfinite(c) and np.isfinite(px).all() and np.isfinite(py).all() else None


def _normal(p, geo, u, v, X, Y):
    px, py, _, J = _model(p, *geo, u, v, jac=True)
    if not (np.isfinite(px).all() and np.isfinite(py).all()):
        return None
    Jf = np.concatenate([J[0], J[1]])
    r = np.concatenate([px - X, py - Y])
    return Jf.T @ Jf, Jf.T @ r


def _solve(A, b, pivot):
    """The unit-diagonal Cholesky's pivot rule, then numpy's solver."""
    dg = np.diag(A)
    if not (np.isfinite(dg).all() and (dg > 0).all()):
        return None
    d = 1.0 / np.sqrt(dg)
    S = A * d[:, None] * d[None, :]
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return None
    if not (np.diag(L) ** 2 > pivot).all():
        return None
    x = np.linalg.solve(S, b * d) * d
    return x if np.isfinite(x).all() else None


def _iterate(p, geo, u, v, X, Y, iters):
    cost = _cost(p, geo, u, v, X, Y)
    if cost is None:
        return None
    lam = LAMBDA0
    for _ in range(iters):
        if cost == 0.0:
            break
        ne = _normal(p, geo, u, v, X, Y)
        if ne is None:
            return None
        A, g = ne
        step = _solve(A + lam * np.diag(np.diag(A)), -g, 0.0)
        if step is None:
            return None
        c2 = _cost(p + step, geo, u, v, X, Y)
        if c2 is not None and c2 < cost:
            done = cost - c2 <= REL_STOP * cost
            p, cost = p + step, c2
            lam = max(lam / 10.0, LAMBDA_MIN)
            if done:
                break
        else:
            lam *= 10.0
            if lam > LAMBDA_MAX:
                break
    ne = _normal(p, geo, u, v, X, Y)
    if ne is None or _solve(ne[0], -ne[1], PIVOT) is None:
        return None
    return p


def placement_lens(sm, cell, aw, ah, min_count, cx, cy, f, order, trim_px, rounds, iters, guard=True):
    """-> None (refused) or dict(k=(k1, k2), quad [4, 2] ideal, H [3, 3] unit slide -> ideal pixels, kept [(cy, cx)], rms, R2: the
    largest r2 of the kept cells' ideal points)."""
    assert (sm.shape[2], sm.shape[1]) == P.E.grid(aw, ah, cell) and min_count >= 1 and trim_px > 0 and 0 <= rounds <= 8 and order in (1, 2)
    cells, u, v, X, Y = P.points(sm, min_count)
    s = float(max(aw, ah))
    geo = (s, float(cx), float(cy), 1.0 / (float(f) * float(f)))
    need = 4 + order
    keep = np.ones(len(cells), bool)
    if keep.sum() < need:
        return None
    H = P._fit(u, v, X, Y, s)
    if H is None:
        return None
    p = np.concatenate([H.reshape(9)[:8], np.zeros(order)])
    p = _iterate(p, geo, u, v, X, Y, iters)
    if p is None:
        return None

    def residuals():
        px, py, _ = _model(p, *geo, u, v)
        with np.errstate(all="ignore"):
            r = np.sqrt((px - X) ** 2 + (py - Y) ** 2)
        return np.where(np.isfinite(r), r, np.inf)
    for _ in range(rounds):
        r = residuals()
        if guard:
            assert (np.abs(r[keep] - trim_px) > P.TRIM_GUARD).all(), "a cell residual lies within %g px of trim_px" % P.TRIM_GUARD
        new = keep & (r <= trim_px)
        if new.sum() == keep.sum():
            break
        keep = new
        if keep.sum() < need:
            return None
        p = _iterate(p, geo, u[keep], v[keep], X[keep], Y[keep], iters)
        if p is None:
            return None
    r = residuals()[keep]
    if not np.isfinite(r).all():
        return None
    R2 = float(_model(p, *geo, u[keep], v[keep])[2].max())
    k1, k2 = float(p[8]), float(p[9]) if order == 2 else 0.0
    if not monotone(k1, k2, R2):
        return None
    Hs = np.append(p[:8], 1.0).reshape(3, 3)
    q = np.stack(P.apply(Hs, s, np.array([0.0, 1, 1, 0]), np.array([0.0, 0, 1, 1])), 1)
    if not np.isfinite(q).all():
        return None
    Hp = Hs.copy()
    Hp[:2] *= s
    return dict(k=(k1, k2), quad=q, H=Hp, kept=[c for c, kk in zip(cells, keep) if kk], rms=float(np.sqrt((r ** 2).mean())), R2=R2)


def displacement(f, k1, k2, r2):
    """f r (g - 1): the radial displacement in pixels at the normalised squared radius r2."""
    return f * np.sqrt(r2) * (k1 * r2 + k2 * r2 * r2)


# ---- the scene of "the use" (both test files) ------------------------------------------------------------------------------------------
# placement_ref.keystone_scene seen through the lens k1 = -0.08 at f = half the diagonal (44 px at the corner of 960x540): the ideal
# frames are the keystone scene's, so the slide's corners in IDEAL coordinates are placement_ref.KEYSTONE_QUAD.  The session's
# settings are placement_ref.USE's.  Bounds: twice the figures the CPU restatement of the pipeline gives on this scene, rounded up to
# a whole pixel (tests/test_frame_lens_abi.py test_the_use_on_the_cpu measures and records them): the largest corner error 2.82 px at
# order 1 and 3.15 px at order 2; the error of the radial displacement f r (g - 1) at the frame's corner 4.64 px and 3.22 px.
USE_K1 = -0.08
USE_ITERS = 100
USE_MEASURED = {1: dict(corner_px=2.82, corner_disp_px=4.64), 2: dict(corner_px=3.15, corner_disp_px=3.22)}
USE_BOUNDS = {1: dict(corner_px=6.0, corner_disp_px=10.0), 2: dict(corner_px=7.0, corner_disp_px=7.0)}


def use_scene(synth):
    """-> (pages, the bent frames uint8 [8, 540, 960, 3], truth, the scene's lens (cx, cy, f, k1, k2))."""
    pages, ideal_frames, truth = P.keystone_scene(synth)
    lens = defaults(ideal_frames.shape[2], ideal_frames.shape[1]) + (USE_K1, 0.0)
    return pages, bend(ideal_frames, lens), truth, lens


def corner_displacement_error(lens, k, w, h):
    """|f r (g_k - g_lens)| at the frame's corner pixel (0, 0): how far the learnt terms k = (k1, k2) put that corner from where the
    scene's lens puts it."""
    cx, cy, f = lens[:3]
    r2 = (cx * cx + cy * cy) / (f * f)
    return float(abs(displacement(f, k[0], k[1], r2) - displacement(f, lens[3], lens[4], r2)))


def out_size_of(quad):
    """The rounded mean lengths of the quad's opposite edge pairs, at least 2 (the learners' default output size)."""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    d = lambda a, b: float(np.hypot(*(q[a] - q[b])))
    return max(2, int(round((d(0, 1) + d(3, 2)) / 2))), max(2, int(round((d(0, 3) + d(1, 2)) / 2)))


def sums_of_lens_homography(Ht, lens, aw, ah, cell, n_per_cell, rng, box=(0.0, 0.0, 1.0, 1.0)):
    """placement_ref.sums_of_homography under a lens: every cell whose centre (X, Y) is the DISTORTED image of a unit-slide point
    inside `box` holds n_per_cell copies of one correspondence: the centre and its exact pre-image under D o Ht (D inverted by
    Newton's method on the radius, to machine precision), rounded to 2^-20."""
    cx, cy, f, k1, k2 = lens
    gw, gh = P.E.grid(aw, ah, cell)
    sm = np.zeros((5, gh, gw), np.uint64)
    Hi = np.linalg.inv(Ht)
    for j in range(gh):
        for i in range(gw):
            X, Y = i * cell + cell / 2.0, j * cell + cell / 2.0
            if X >= aw or Y >= ah:
                continue
            rd = np.hypot(X - cx, Y - cy) / f
            r = rd
            for _ in range(60):
                r = r - (r * (1 + k1 * r * r + k2 * r ** 4) - rd) / (1 + 3 * k1 * r * r + 5 * k2 * r ** 4)
            g = 1 + k1 * r * r + k2 * r ** 4
            px, py = cx + (X - cx) / g, cy + (Y - cy) / g
            w = Hi @ np.array([px, py, 1.0])
            u, v = w[0] / w[2], w[1] / w[2]
            if not (box[0] <= u <= box[2] and box[1] <= v <= box[3]):
                continue
            k = int(n_per_cell if np.isscalar(n_per_cell) else rng.integers(n_per_cell[0], n_per_cell[1]))
            sm[:, j, i] = [k, k * int(round(X * 16)), k * int(round(Y * 16)), k * int(round(u * 1048576)), k * int(round(v * 1048576))]
    return sm
