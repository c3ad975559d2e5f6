"""Checks (a)-(f) of the float64 definition tests, shared by the CPU file (the restatement in oracle/) and the GPU file (the HIP
kernels): each takes what an implementation produced and holds it to tests/f64_defs.py.  Each returns the largest deviation it
saw and the counts it checked, for the report line `report` prints (visible with pytest -s)."""
import os

import numpy as np

import f64_defs as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# blur variant (slideo_ocv_variants.blur) -> how far the blurred level may lie from gauss7 of the unblurred one, in grey levels
# (tests/test_oracle_variants.py:66): f32 taps, correctly rounded: 0.5 + f32 error; Q8 taps summing to 257: (257/256)^2
# brighter, <= 2 levels plus rounding; Q8 taps summing to 256: their distance from the float taps plus rounding
BLUR_BOUND = {0: 0.51, 1: 0.51, 2: 2.6, 3: 1.6}
ANGLE_BOUND = 0.02             # fastAtan2's polynomial error, ~0.01 degrees (tests/test_oracle_variants.py:102)


def golden_bgr(name):
    """A committed PNG of tests/golden as a BGR8 image."""
    from PIL import Image
    return np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))[:, :, ::-1])


# the INTER_AREA shapes of the path: factors 4.165, 4.34, 8.33, 2.78, 1.39 and 4 (the integer fast path)
AREA_SHAPES = [(1920, 1080), (2001, 1125), (3840, 2160), (1280, 720), (640, 360), (1600, 1200)]


def area_input(synth, w, h):
    """The INTER_AREA input of a shape: the natural frame and page at their own sizes, synthetic frames and a 4:3 page elsewhere."""
    if (w, h) == (1920, 1080):
        return golden_bgr("2-frame.png")
    if (w, h) == (2001, 1125):
        return golden_bgr("1-slide.png")
    if (w, h) == (1600, 1200):
        return synth.pages(1, 1600, 1200, seed=7)[0]
    return synth.frames(synth.pages(2), 1, w, h, first=4)[0][0]


def orb_inputs(synth):
    """The ORB inputs at the reference's shapes: a synthetic 1080p frame, a 2001x1125 page and the natural 1080p frame."""
    pages = synth.pages(2)
    frames, _, _ = synth.frames(pages, 1, first=1)
    return {"synthetic_1080p": frames[0], "page_2001x1125": pages[1], "natural_1080p": golden_bgr("2-frame.png")}


def report(name, **kv):
    print("F64 %-12s " % name + " ".join("%s=%s" % (k, ("%.4g" % v) if isinstance(v, float) else v) for k, v in kv.items()))


def _orb_lits(cfg):
    return cfg.nfeatures, float(cfg.scale_factor), cfg.nlevels


def check_pyramid(bgr, cfg, level, blurred, blur_variant):
    """(a) level shapes = level_sizes; level 0 within 0.51 of gray (Q15 coefficients: 0.5 rounding + < 0.01); level l within
    1 of bilinear_down of the implementation's own level l - 1 wherever 8.8 fixed-point weights allow it, and everywhere within
    bilinear_q8_bound (the weights' 1/512 error times the local differences, + 0.5: up to 1.5 at a full-range edge); the blurred level
    within BLUR_BOUND of gauss7 of the implementation's own unblurred level.  level(l), blurred(l): the implementation's."""
    h, w, _ = bgr.shape
    ws, hs, _ = D.level_sizes(w, h, cfg.scale_factor, cfg.nlevels)
    L = [level(l) for l in range(cfg.nlevels)]
    assert [x.shape for x in L] == list(zip(hs.tolist(), ws.tolist()))
    d0 = np.abs(L[0] - D.gray(bgr)).max()
    assert d0 <= 0.51, d0
    dl, over1 = 0.0, 0
    for l in range(1, cfg.nlevels):
        d = np.abs(L[l] - D.bilinear_down(L[l - 1], ws[l], hs[l]))
        bound = D.bilinear_q8_bound(L[l - 1], ws[l], hs[l])
        assert (d <= bound).all(), (l, d.max(), (d - bound).max())
        assert (d[bound <= 1.0] <= 1.0).all()
        dl = max(dl, d.max()); over1 += int((d > 1.0).sum())
    db = 0.0
    for l in range(cfg.nlevels):
        B = blurred(l)
        assert B.shape == L[l].shape
        d = np.abs(B - D.gauss7(L[l])).max()
        assert d <= BLUR_BOUND[blur_variant], (l, d)
        db = max(db, d)
    report("pyramid", gray=d0, linear=dl, linear_over_1=over1, blur=db, blur_bound=BLUR_BOUND[blur_variant])
    return L


def kp_level_xy(kp, scales):
    """Integer level coordinates of keypoints; each must lie on a level pixel within 1e-3 after dividing by the level scale."""
    s = scales[kp["octave"]].astype(np.float64)
    xl = kp["x"].astype(np.float64) / s
    yl = kp["y"].astype(np.float64) / s
    xi, yi = np.rint(xl), np.rint(yl)
    dev = max(np.abs(xl - xi).max(initial=0), np.abs(yl - yi).max(initial=0))
    assert dev <= 1e-3, dev
    return xi.astype(np.int64), yi.astype(np.int64), dev


def check_detection(cfg, L, kp):
    """(b) per level: S = the corners of fast_nms(fast_score(level)) at least edge_threshold inside the level (none when the
    level is not larger than 2 edge_threshold, runByImageBorder); K = the keypoints of that octave, thr = their smallest
    response.  K == {p in S : score >= thr}, response == score, and retainBest: if |S| > quota then #{score > thr} < quota <=
    #{score >= thr}, else K == S."""
    nf, sf, nl = _orb_lits(cfg)
    quota = D.level_quotas(nf, sf, nl)
    _, _, scales = D.level_sizes(L[0].shape[1], L[0].shape[0], sf, nl)
    xi, yi, dev = kp_level_xy(kp, scales)
    e = cfg.edge_threshold
    nS = nK = 0
    for l in range(nl):
        lh, lw = L[l].shape
        sc = D.fast_score(L[l], cfg.fast_threshold)
        keep = D.fast_nms(sc)
        if lw <= 2 * e or lh <= 2 * e:
            keep[:] = False
        else:
            keep[:e] = False; keep[lh - e:] = False; keep[:, :e] = False; keep[:, lw - e:] = False
        sy, sx = np.nonzero(keep)
        S = dict(zip(zip(sx.tolist(), sy.tolist()), sc[sy, sx].tolist()))
        sel = kp["octave"] == l
        K = list(zip(xi[sel].tolist(), yi[sel].tolist()))
        resp = kp["response"][sel]
        assert len(set(K)) == len(K), "duplicate keypoints in octave %d" % l
        assert all(p in S for p in K), "octave %d: keypoints that are not corners" % l
        assert np.array_equal(resp, np.array([S[p] for p in K], np.float32)), "octave %d: response != score" % l
        if not K:
            assert not S or quota[l] == 0, (l, len(S), quota[l])
        else:
            thr = resp.min()
            want = {p for p, s in S.items() if s >= thr}
            assert set(K) == want, "octave %d: %d keypoints, %d corners score >= %g" % (l, len(K), len(want), thr)
            if len(S) > quota[l]:
                above = sum(s > thr for s in S.values())
                assert above < quota[l] <= len(K), (l, above, quota[l], len(K))
            else:
                assert len(K) == len(S)
        nS += len(S); nK += len(K)
    assert nK == len(kp)
    report("detection", keypoints=nK, corners=nS, pos_dev=dev)
    return xi, yi


def check_angles(cfg, L, kp, xi, yi):
    """(c) every keypoint's angle within ANGLE_BOUND degrees (mod 360) of ic_angle on the UNBLURRED level."""
    half = cfg.patch_size // 2
    worst = 0.0
    for l in range(cfg.nlevels):
        sel = kp["octave"] == l
        if not sel.any():
            continue
        ref = D.ic_angle(L[l], xi[sel], yi[sel], half)
        d = np.abs(kp["angle"][sel].astype(np.float64) - ref) % 360.0
        d = np.minimum(d, 360.0 - d)
        worst = max(worst, d.max())
    assert worst <= ANGLE_BOUND, worst
    report("angle", max_dev=worst, bound=ANGLE_BOUND, keypoints=len(kp))


def check_descriptors(cfg, B, kp, desc, xi, yi, pattern):
    """(d) every non-ambiguous bit equals brief() computed with the implementation's own angle on its own blurred level; at most
    0.5 % of the bits are ambiguous (either sample within BRIEF_MARGIN of a rounding boundary)."""
    got = D.unpack_descriptors(desc)
    bad = amb_n = 0
    for l in range(cfg.nlevels):
        sel = np.nonzero(kp["octave"] == l)[0]
        if not len(sel):
            continue
        bits, amb = D.brief(B[l], xi[sel], yi[sel], kp["angle"][sel], pattern)
        bad += int(((bits != got[sel]) & ~amb).sum())
        amb_n += int(amb.sum())
    total = max(len(kp) * 256, 1)
    assert bad == 0, "%d non-ambiguous descriptor bits differ" % bad
    assert amb_n / total <= 0.005, amb_n / total
    report("descriptor", bits=total, ambiguous_frac=amb_n / total, wrong=bad)


def check_orb(bgr, cfg, blur_variant, level, blurred, kp, desc, pattern):
    """(a)-(d) on one image.  level(l) / blurred(l): the implementation's pyramid; kp, desc: its ORB output."""
    L = check_pyramid(bgr, cfg, level, blurred, blur_variant)
    B = [blurred(l) for l in range(cfg.nlevels)]
    xi, yi = check_detection(cfg, L, kp)
    check_angles(cfg, L, kp, xi, yi)
    check_descriptors(cfg, B, kp, desc, xi, yi, pattern)
    assert len(kp) > 0


def check_area(small, src, small_area=120000):
    """(e) INTER_AREA to the small size: the shape is small_size's; every channel within 0.5 + eta (< 1) of the exact box mean;
    equal to rint(mean) wherever the mean is farther than eta (area_eta) from a rounding boundary, and on at least 99 % of all
    channels (a sharpness guard: eta must not swallow the check)."""
    h, w = src.shape[:2]
    sw, sh = D.small_size(w, h, small_area)
    assert small.shape == (sh, sw, 3), (small.shape, sw, sh)
    mean, _, _ = D.area_resize(src, sw, sh)
    eta = D.area_eta(w, h, sw, sh)[:, :, None]
    dev = np.abs(small - mean)
    assert (dev <= 0.5 + eta).all(), dev.max()
    far = np.abs(mean - np.floor(mean) - 0.5) > eta
    exact = small == np.rint(mean)
    assert exact[far].all(), "%d channels away from a rounding boundary differ" % (~exact & far).sum()
    assert exact.mean() >= 0.99, exact.mean()
    report("area", size="%dx%d->%dx%d" % (w, h, sw, sh), max_dev=float(dev.max()), eta_max=float(eta.max()), exact=float(exact.mean()))


def check_reprojection(frame, cands, page_shapes, page_small, stats):
    """(f) every candidate with similarity != 0: |similarity - reprojection_similarity| <= similarity_bound, with the candidate's
    recorded transform and the implementation's page small image.  stats: a dict that collects counts and deviations.

    For the sharpness guard (`sharp` of `regular`) a candidate whose map is COLLAPSED (linear scale below 0.1: RANSAC's fit to a
    wrong page, the whole page drawn from a few frame pixels, so that whole page rows share one half-pixel rounding decision) is
    counted apart; it is held to its bound all the same."""
    for c in cands:
        if c["similarity"] == 0:
            continue
        ph, pw = page_shapes[c["page_idx"]]
        M = np.asarray(c["transform"], np.float64).reshape(3, 3)
        rep = D.reprojection(frame, M, pw, ph)
        want = D.reprojection_similarity(frame, M, pw, ph, page_small[c["page_idx"]], rep=rep)
        bound = D.similarity_bound(frame, M, pw, ph, page_small[c["page_idx"]], rep=rep)
        d = abs(float(c["similarity"]) - want)
        assert d <= bound, (int(c["page_idx"]), float(c["similarity"]), want, bound)
        stats["n"] = stats.get("n", 0) + 1
        if np.sqrt(abs(np.linalg.det(M[:2, :2]))) < 0.1 * abs(M[2, 2]):
            stats["collapsed"] = stats.get("collapsed", 0) + 1
        else:
            stats["regular"] = stats.get("regular", 0) + 1
            stats["sharp"] = stats.get("sharp", 0) + int(bound < 1e-3)
        stats["max_dev"] = max(stats.get("max_dev", 0.0), d)
        stats["max_bound"] = max(stats.get("max_bound", 0.0), bound)
        stats["amb"] = stats.get("amb", 0) + int((rep[1] > 0).sum())
        stats["chan"] = stats.get("chan", 0) + rep[1].size


# ---- SIFT (tests/f64_defs_sift.py) -------------------------------------------------------------------------------------------
# Each check takes its input from the tested implementation's own upstream output (its gray image, its previous layer, its DoG
# layers, its keypoints), so that errors do not compound and every discrete decision on f32 inputs is exact.

import f64_defs_sift as S  # noqa: E402

U32 = 2.0 ** -24               # unit round-off of f32

# Boundary width of the refinement's decisions (S.refine's margin): a candidate whose every decision is farther than this from
# its boundary must come out the same in f32.  It has to exceed the f32 error of what is compared: the offsets carry the
# solve's error, at most 8 SOLVE_K = 1.3e-4 pixels (below); the contrast and edge tests compare sums of a few f32 products,
# relative error of some 10 u = 6e-7 plus the solve's share.  1e-3 is above both with room; what it excuses is capped below.
SIFT_BOUNDARY = 1e-3
SIFT_UNDECIDED_CAP = 0.02      # share of refined candidates per image that may lie within SIFT_BOUNDARY of a decision
# The error of the 3 x 3 solve in f32: the largest |offset(f32) - offset(f64)| of S.refine evaluated in np.float32 against the
# same definition in float64, over every accepted candidate of inputs A, B and C (sift_inputs): 1.6e-5 pixels (measured by
# sift_solve_constant; tests/test_oracle_sift_definitions.py asserts that the measurement stays below this constant).  An
# implementation orders the operations of its solve differently (Cramer's rule by cofactors), hence a margin of 8 x wherever
# the constant is used.
SOLVE_K = 5e-7
SOLVE_MARGIN = 8.0
# The error of a sample's gradient angle.  OpenCV documents fastAtan2 as accurate to "about 0.3 degrees", a figure that dates
# from its table-driven version; the routine of OpenCV 3 and 4 is a 7th-degree odd polynomial whose error stays below 0.02
# degrees (tests/test_oracle_variants.py holds the routine in use to that against atan2).  The bounds below propagate the
# WORST case of this error (every sample off by the full amount, in the most harmful direction).  Propagated that way, 0.3
# degrees allows descriptor elements to move by up to 9 and half of the orientation peaks by more than 2.5 degrees (measured on
# the definition's own histograms of inputs A to C): no wrong bin or weight could be told from it.  0.02 is the sharper of
# the two and the one that holds for the polynomial.
ATAN_ERR = 0.02
PEAK_MARGIN = 0.002            # a peak is decided when it clears both neighbours and 0.8 max by this share of max
PEAK_UNDECIDED_CAP = 0.03
ANGLE_CAP = 3.0                # degrees; no angle bound is wider than this, whatever peak_angle_bound derives: well below the 10 degree bin


def sift_inputs():
    """The SIFT inputs: A a natural crop 320 x 240, B noise 131 x 97, C a natural crop 277 x 189 at sigma 1.55 (a 25-tap blur);
    and the small images of the kernel-path sweep.  name -> (bgr, sigma)."""
    full = golden_bgr("2-frame.png")
    rng = np.random.default_rng(5)
    return {"A": (np.ascontiguousarray(full[300:540, 600:920]), 1.6),
            "B": (rng.integers(0, 256, (97, 131, 3), dtype=np.uint8), 1.6),
            "C": (np.ascontiguousarray(full[200:389, 500:777]), 1.55)}


# The kernel-path sweep: sigmas in (0.5, 2.4] whose blurs, over the sweep images, take every tap count of the product's unrolled
# blur kernel (7 to 27, odd, on layers at least 32 x 32) and 29, 33 and 39 taps on its generic one.  The tap counts are
# S.blur_plan's; the tests assert the coverage.
SIFT_SWEEP_SIGMAS = (0.6, 1.75, 2.0, 2.4)


def sift_sweep_taps(sigmas=SIFT_SWEEP_SIGMAS):
    """(tap counts on layers of at least 32 x 32 with 7 .. 27 taps, tap counts on every other layer) over the sweep."""
    unrolled, generic = set(), set()
    for bgr in sift_sweep_images().values():
        for sg in sigmas:
            for _, _, n, lw, lh in S.blur_plan(bgr.shape[1], bgr.shape[0], sg):
                (unrolled if lw >= 32 and lh >= 32 and 7 <= n <= 27 else generic).add(n)
    return unrolled, generic


def sift_sweep_images():
    """33 x 40 (doubled 66 x 80: a 2-column last strip, rows no multiple of 8, octave 1 at the 32-pixel switch, octave 2 below
    it), 16 x 17 (doubled exactly 32 wide) and 131 x 97, all noise.  name -> bgr."""
    rng = np.random.default_rng(17)
    return {"33x40": rng.integers(0, 256, (40, 33, 3), dtype=np.uint8), "16x17": rng.integers(0, 256, (17, 16, 3), dtype=np.uint8),
            "131x97": rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)}


def blur_bound(taps, src_max):
    """How far an f32 separable blur may lie from S.blur of the same source.  Row pass: taps products accumulated one after the
    other, each operation within u of exact: taps u.  Column pass: the centre product plus taps // 2 pair sums, each a sum and a
    multiply-add: (taps + 1) u.  The taps themselves are f32: u on each pass.  Every partial sum is at most max|src| (the taps
    are positive and sum to 1), so the total is (2 taps + 4) u max|src| to first order."""
    return (2 * taps + 4) * U32 * src_max


def check_sift_pyramid(gray8, sigma, layer, n_octaves=None, name=""):
    """layer(o, i, dog): the tested Gaussian / DoG layer.  Sizes and octave count are S.octave_sizes'; layer (0, 0) within
    blur_bound (+ 4 u 255 for the two f32 interpolations of the upsample) of S.base_image of the tested gray image; every other
    layer within blur_bound of S.blur of the tested previous layer; octave o + 1 starts with every second pixel of layer 3 of
    octave o and every DoG layer is the f32 difference of its two Gaussian layers, both exactly.
    -> (G, DoG): per octave the lists of float32 layers."""
    h, w = gray8.shape
    sizes = S.octave_sizes(w, h)
    if n_octaves is not None:
        assert n_octaves == len(sizes), (n_octaves, len(sizes))
    sig = S.layer_sigmas(sigma)
    G, DOG, worst = [], [], 0.0
    for o, shape in enumerate(sizes):
        g = [layer(o, i, False) for i in range(S.NL + 3)]
        assert all(x.shape == shape and x.dtype == np.float32 for x in g), (o, [x.shape for x in g], shape)
        if o == 0:
            taps = S.num_taps(S.base_sigma(sigma))
            bound = blur_bound(taps, 255.0) + 4 * U32 * 255.0
            d = np.abs(g[0] - S.base_image(gray8, sigma)).max()
            assert d <= bound, ("base", d, bound)
            worst = max(worst, d / bound)
        else:
            assert np.array_equal(g[0], G[o - 1][S.NL][::2, ::2][:shape[0], :shape[1]]), ("octave step", o)
        for i in range(1, S.NL + 3):
            bound = blur_bound(S.num_taps(sig[i - 1]), float(np.abs(g[i - 1]).max()))
            d = np.abs(g[i] - S.blur(g[i - 1], sig[i - 1])).max()
            assert d <= bound, ("blur", o, i, d, bound)
            worst = max(worst, d / bound)
        dog = [layer(o, i, True) for i in range(S.NL + 2)]
        for i in range(S.NL + 2):
            assert dog[i].dtype == np.float32 and np.array_equal(dog[i], g[i + 1] - g[i]), ("dog", o, i)
        G.append(g); DOG.append(dog)
    report("sift-pyramid", image=name, sigma=sigma, octaves=len(sizes), blur_observed_over_bound=worst)
    return G, DOG


def sift_octave(field):
    """Pyramid octave index (0 = the doubled image) of a keypoint's octave field."""
    o = np.asarray(field).astype(np.int64) & 255
    return np.where(o >= 128, o - 256, o) + 1


def sift_candidates(DOG, sigma, ct=0.04, et=10.0, dtype=np.float64):
    """The definition's refined candidates from DoG layers: (number of raw extrema, {(octave, layer, r, c): S.refine record}).
    Two extrema that refine to the same place are one candidate (the better margin is kept)."""
    n_raw, cands = 0, {}
    for o, dog in enumerate(DOG):
        d64 = [x.astype(np.float64) for x in dog]
        for l in range(1, S.NL + 1):
            rr, cc = S.raw_extrema(dog[l - 1], dog[l], dog[l + 1], ct)
            n_raw += len(rr)
            for r, c in zip(rr.tolist(), cc.tolist()):
                rec = S.refine(d64, l, r, c, o, sigma, ct, et, dtype=dtype)
                if rec is None:
                    continue
                key = (o, rec["layer"], rec["r"], rec["c"])
                if key not in cands or cands[key]["margin"] < rec["margin"]:
                    cands[key] = rec
    return n_raw, cands


def sift_solve_constant(DOG, sigma):
    """Largest |offset| difference between S.refine in np.float32 and in float64 over the accepted, decided candidates."""
    _, c64 = sift_candidates(DOG, sigma)
    _, c32 = sift_candidates(DOG, sigma, dtype=np.float32)
    worst = 0.0
    for key, a in c64.items():
        if a["accepted"] and a["margin"] > SIFT_BOUNDARY and key in c32:
            worst = max(worst, np.abs(a["off"] - c32[key]["off"]).max())
    return worst


def sift_kp_bounds(rec, octave):
    """Bounds of a refined keypoint's fields against the S.refine record, with e = SOLVE_MARGIN SOLVE_K, the solve's f32 error
    in octave pixels, and s = 2^octave / 2 the octave's scale in the input image.
    x, y: the coordinate is one f32 sum c + xc (within u of its value; the scaling by powers of two is exact), xc itself an f32
    quotient (u / 2): u (|x| + s) + e s.
    size: sigma 2^((layer + xi) / 3) 2 s in f32: sigma's conversion, the sum, the quotient, the power and two products, each
    within u, the exponent's two weighed by ln 2 (layer + xi) / 3 < 1: 8 u relative covers them; xi's error e moves the
    exponent by e / 3: ln 2 / 3 e < e / 4 relative.
    response: |v / 255 + (g . off) / 2|: the quotient and each product and sum within u of terms that sum to
    resp_terms = |v| / 255 + sum |g_i off_i|: 8 u resp_terms; the offsets' error e enters through g: e / 2 sum |g_i|.
    xi byte: cvRound((xi + 0.5) 255) moves by at most one for an xi error far below 1 / 255."""
    e = SOLVE_MARGIN * SOLVE_K
    s = 2.0 ** octave * 0.5
    return dict(x=U32 * (abs(rec["x"]) + s) + e * s, y=U32 * (abs(rec["y"]) + s) + e * s,
                size=rec["size"] * (8 * U32 + e / 4), response=8 * U32 * rec["resp_terms"] + 0.5 * e * rec["grad_l1"], xi_byte=1)


def check_sift_keypoints(DOG, kp, sigma, ct=0.04, et=10.0, n_raw=None, n_refined=None, name=""):
    """DOG: the tested DoG layers; kp: the tested keypoints (nfeatures = 0).  The raw extrema are S.raw_extrema of the tested
    layers (exact comparisons; n_raw: the tested count where the implementation exposes it).  Every candidate of S.refine that
    is accepted with a margin above SIFT_BOUNDARY appears among the tested keypoints with every field within sift_kp_bounds;
    every tested keypoint is a candidate (decided or not) within the same bounds; at most SIFT_UNDECIDED_CAP of the candidates
    are undecided.  -> the tested refined points: [(octave, layer, r, c, size, [indices into kp])]."""
    n_def, cands = sift_candidates(DOG, sigma, ct, et)
    if n_raw is not None:
        assert n_raw == n_def, ("raw extrema", n_raw, n_def)
    decided = {k for k, v in cands.items() if v["accepted"] and v["margin"] > SIFT_BOUNDARY}
    undecided = {k for k, v in cands.items() if v["margin"] <= SIFT_BOUNDARY}
    share = len(undecided) / max(len(decided) + len(undecided), 1)
    assert share <= SIFT_UNDECIDED_CAP, ("undecided share", len(undecided), len(decided))
    # the tested keypoints, one group per refined point (a point has one keypoint per orientation peak)
    groups = {}
    for i, q in enumerate(kp):
        groups.setdefault((int(q["octave"]), float(q["x"]), float(q["y"]), float(q["size"]), float(q["response"])), []).append(i)
    if n_refined is not None:
        assert n_refined >= len(groups), (n_refined, len(groups))
    by_layer = {}
    for key in cands:
        by_layer.setdefault(key[:2], []).append(key)
    worst = dict(x=0.0, y=0.0, size=0.0, response=0.0)
    seen, points = set(), []
    for (field, x, y, size, resp), idx in groups.items():
        o, layer = int(sift_octave(field)), (field >> 8) & 255
        hit = None
        for key in by_layer.get((o, layer), []):
            rec = cands[key]
            if key not in decided and key not in undecided:
                continue                                        # decidedly rejected
            b = sift_kp_bounds(rec, o)
            if abs(x - rec["x"]) <= b["x"] and abs(y - rec["y"]) <= b["y"]:
                hit = key
                break
        assert hit is not None, "tested keypoint at (%.4f, %.4f) octave %d layer %d is no refined candidate" % (x, y, o, layer)
        assert hit not in seen, ("two tested points at one candidate", hit)
        seen.add(hit)
        rec, b = cands[hit], sift_kp_bounds(cands[hit], o)
        assert abs(size - rec["size"]) <= b["size"], ("size", hit, size, rec["size"], b["size"])
        assert abs(resp - rec["response"]) <= b["response"], ("response", hit, resp, rec["response"], b["response"])
        assert field & 0xffff == rec["octave_field"] & 0xffff and abs((field >> 16) - rec["xi_byte"]) <= b["xi_byte"], ("octave", hit, field)
        for f, v in (("x", x), ("y", y), ("size", size), ("response", resp)):
            worst[f] = max(worst[f], abs(v - rec[f]) / b[f])
        points.append((o, layer, hit[2], hit[3], size, idx))
    missing = decided - seen
    assert not missing, "%d decided keypoints missing, e.g. %s" % (len(missing), sorted(missing)[:3])
    report("sift-keypoints", image=name, raw=n_def, points=len(groups), decided=len(decided), undecided=len(undecided),
           undecided_share=share, **{"%s_observed_over_bound" % f: v for f, v in worst.items()})
    return points


def _angle_dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - b) % 360.0
    return np.minimum(d, 360.0 - d)


def peak_angle_bound(hist, slack, j):
    """How far the interpolated angle of peak j may move when every histogram value moves by at most its slack (the samples
    that ATAN_ERR may put into the neighbouring bin and the 2^-21 rounding of every fixed-point vote, S.orientation_hist) plus
    the f32 round-off of the sums and of the smoothing (64 u max, generously): the offset p = (l - r) / 2 (l - 2 c + r) has a
    numerator error dn <= sl + sr and a denominator error dd <= sl + 2 sc + sr, so |dp| <= (dn / 2 + |p| dd) / (|den| - dd), in
    bins of 10 degrees.  inf when the slack can cancel the curvature (a flat peak)."""
    n = len(hist)
    l, c, r = hist[(j - 1) % n], hist[j], hist[(j + 1) % n]
    f32 = 64 * U32 * hist.max()                                 # the fixed-point / f32 sums and the smoothing, generously
    sl, sc, sr = slack[(j - 1) % n] + f32, slack[j] + f32, slack[(j + 1) % n] + f32
    den = abs(l - 2 * c + r)
    dd = sl + 2 * sc + sr
    if den <= dd:
        return np.inf
    p = abs(0.5 * (l - r) / (l - 2 * c + r))
    return (360.0 / n) * (0.5 * (sl + sr) + p * dd) / (den - dd)


def check_sift_orientation(G, kp, points, name=""):
    """points: check_sift_keypoints' tested refined points.  Per point the definition histogram on the tested Gaussian layer at
    the tested (r, c) and scale (size / 2^octave).  A definition peak is decided when its margin exceeds PEAK_MARGIN.  Every
    decided peak has a tested angle within min(peak_angle_bound, ANGLE_CAP); every tested angle has a definition peak or
    near-peak (margin > -PEAK_MARGIN) within the same; at most PEAK_UNDECIDED_CAP of the peaks are undecided.  Where the
    derived bound is wider than ANGLE_CAP (a flat peak) the cap is what is asserted: stricter than derived."""
    n_dec = n_und = 0
    worst = worst_deg = widest = 0.0
    for o, layer, r, c, size, idx in points:
        L = G[o][layer].astype(np.float64)
        hist, slack = S.orientation_hist(L, r, c, size / 2.0 ** o, ATAN_ERR, 2.0 ** -21)
        peaks = [(a, m, peak_angle_bound(hist, slack, j)) for a, j, m in S.orientation_peaks(hist, PEAK_MARGIN)]
        got = kp["angle"][idx].astype(np.float64)
        assert ((got >= 0) & (got < 360)).all()
        for a, m, b in peaks:
            b = min(b, ANGLE_CAP)
            if m > PEAK_MARGIN:
                d = _angle_dist(got, a).min()
                assert d <= b, ("peak at %.3f deg of point %s: nearest tested angle %.3f away, bound %.3f" % (a, (o, layer, r, c), d, b))
                n_dec += 1; worst = max(worst, d / b); worst_deg = max(worst_deg, d); widest = max(widest, b)
            elif m > 0:
                n_und += 1
        for t in got:
            assert any(_angle_dist(t, a) <= min(b, ANGLE_CAP) for a, m, b in peaks), ("tested angle %.3f of point %s is no peak" % (t, (o, layer, r, c)))
    share = n_und / max(n_dec + n_und, 1)
    assert share <= PEAK_UNDECIDED_CAP, ("undecided peaks", n_und, n_dec)
    report("sift-orientation", image=name, points=len(points), decided=n_dec, undecided=n_und, undecided_share=share,
           angle_observed_over_bound=worst, max_angle_dev=worst_deg, widest_bound=widest)


def descriptor_delta(v, det):
    """delta(v) per element: how far the implementation's unrounded value may lie from the definition's v.
    (1) the angle: an error of ATAN_ERR degrees is ATAN_ERR / 45 of an orientation bin; the trilinear orientation weight
        has slope 1 per bin, so each sample moves at most that share of its spatially weighted magnitude into or out of an
        element: (ATAN_ERR / 45) support, in raw units.
    (2) the fixed-point sums: every vote is rounded to 2^-20, half a quantum each: votes 2^-21.
    (3) f32: the vote weights are a few f32 products (16 u relative of the sum covers them).
    In output units these are scaled by k = 512 / clamped_norm.  The clamp level and the final norm follow the raw vector's
    norm, which moves by at most the norm of the raw errors, relatively rel = |errors| / norm: v (2 rel + 8 u) more."""
    raw_err = (ATAN_ERR / 45.0) * det["support"] + det["votes"] * 2.0 ** -21 + 16 * U32 * det["raw"]
    k = S.D_SCALE / det["clamped_norm"]
    rel = np.linalg.norm(raw_err) / max(det["norm"], 1e-300)
    return k * raw_err + v * (2 * rel + 8 * U32)


def check_sift_descriptors(G, kp, desc, name=""):
    """Per tested keypoint the definition descriptor at the tested position, angle and size on the tested Gaussian layer:
    |byte - clip(v, 0, 255)| <= 0.5 + delta(v) for every element, and delta < 1 for every element that occurs (so that a vote
    in the wrong bin or with a wrong weight cannot hide)."""
    assert desc.shape == (len(kp), 128) and desc.dtype == np.uint8
    worst = worst_dev = worst_delta = 0.0
    differ = 0
    for q, got in zip(kp, desc):
        o, layer = int(sift_octave(q["octave"])), (int(q["octave"]) >> 8) & 255
        s = 2.0 / 2.0 ** o                                       # input image -> octave coordinates
        ori = (360.0 - float(q["angle"])) % 360.0
        v, det = S.descriptor(G[o][layer].astype(np.float64), float(q["x"]) * s, float(q["y"]) * s, ori, float(q["size"]) * s * 0.5,
                              detail=True, atan_err=ATAN_ERR)
        delta = descriptor_delta(v, det)
        assert delta.max() < 1.0, ("delta", delta.max())
        dev = np.abs(got.astype(np.float64) - np.clip(v, 0, 255))
        bad = dev > 0.5 + delta
        assert not bad.any(), ("descriptor of keypoint at (%.2f, %.2f): element %d is %d, definition %.3f, delta %.3f"
                               % (q["x"], q["y"], int(np.argmax(bad)), got[np.argmax(bad)], v[np.argmax(bad)], delta[np.argmax(bad)]))
        worst = max(worst, ((dev - 0.5) / (delta + 1e-300)).max()); worst_dev = max(worst_dev, dev.max()); worst_delta = max(worst_delta, delta.max())
        differ += int((got != np.clip(np.floor(v + 0.5), 0, 255)).sum())
    report("sift-descriptor", image=name, keypoints=len(kp), max_abs_v_minus_byte=worst_dev, excess_over_delta=worst,
           max_delta=worst_delta, differing_bytes_per_descriptor=differ / max(len(kp), 1))


def sift_keys(kp):
    """Canonical keys of tested keypoints from their own fields: row and column are the rounded octave coordinates, the peak
    bin the rounded (360 - angle) / 10."""
    o = sift_octave(kp["octave"])
    layer = (kp["octave"].astype(np.int64) >> 8) & 255
    s = 2.0 / 2.0 ** o
    c = np.rint(kp["x"].astype(np.float64) * s).astype(np.int64)
    r = np.rint(kp["y"].astype(np.float64) * s).astype(np.int64)
    b = np.rint((360.0 - kp["angle"].astype(np.float64)) / 10.0).astype(np.int64) % S.BINS
    return S.canonical_keys(o, layer, r, c, b)


def check_sift_selection(sift, ns, name=""):
    """sift(n) -> (kp, desc) of the tested implementation for nfeatures = n.  sift(n) is sift(0) filtered by S.retain_best, and
    both are in canonical order.  ns: the nfeatures to try; a value whose n-th response is tied is added when the image has
    one."""
    kp0, d0 = sift(0)
    keys = sift_keys(kp0)
    assert all(a < b for a, b in zip(keys, keys[1:])), "nfeatures=0 is not in canonical order"
    resp = np.sort(kp0["response"])[::-1]
    ties = [i + 1 for i in range(len(resp) - 1) if resp[i] == resp[i + 1] and (i == 0 or resp[i - 1] != resp[i])]
    tied = 0
    for n in list(ns) + ties[:1]:
        kpn, dn = sift(n)
        keep = S.retain_best(kp0["response"], n)
        assert len(kpn) == keep.sum() >= min(n, len(kp0)), (n, len(kpn), int(keep.sum()))
        assert np.array_equal(kpn, kp0[keep]) and np.array_equal(dn, d0[keep]), n
        kn = sift_keys(kpn)
        assert all(a < b for a, b in zip(kn, kn[1:])), n
        tied += int(keep.sum() > n)
    report("sift-selection", image=name, keypoints=len(kp0), nfeatures=list(ns) + ties[:1], kept_beyond_n=tied)


def check_sift(bgr, gray8, sigma, sift, layer, stats=None, name=""):
    """All SIFT checks on one image.  sift(n) -> (kp, desc); layer(o, i, dog) -> the tested layer; stats: the implementation's
    own counts (octaves, extrema, refined) where it has them."""
    stats = stats or {}
    G, DOG = check_sift_pyramid(gray8, sigma, layer, stats.get("octaves"), name)
    kp, desc = sift(0)
    points = check_sift_keypoints(DOG, kp, sigma, n_raw=stats.get("extrema"), n_refined=stats.get("refined"), name=name)
    check_sift_orientation(G, kp, points, name)
    check_sift_descriptors(G, kp, desc, name)
    return G, DOG, kp, desc, points
