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
