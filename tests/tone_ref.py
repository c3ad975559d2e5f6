"""The match tone table (include/slideo_amd.h "Match tone table") restated in numpy, written from the header: the counts of a batch of
frames from their keypoints, their votes, their candidate records, the analysed images and the pages' small images, in float64; the
table made of count arrays, in Python integers.  Nothing here calls the library.

A frame is a dict: xy float32 [K, 2] (the keypoints), votes [(q, t)] (query in frame, train row: every vote of the frame, any
order), cands [(page, inliers, transform (9 values))] in slot order (the trace's candidates), image uint8 [ah, aw, 3] (the analysed
frame).  pages: {page: (w, h, small uint8 [sh, sw, 3])}."""
import numpy as np

import evidence_ref as E

MAX_FRAMES = 1 << 31
GUARD = 1e-9          # no tested value may lie within this of its threshold / of an integer: a condition on the INPUTS


def contributor(cands, min_inliers):
    """The slot of the contributor among [(page, inliers, transform)], or -1."""
    best = -1
    for j, (_, inl, M) in enumerate(cands):
        if not np.any(np.asarray(M, np.float64) != 0) or inl < min_inliers:
            continue
        if best < 0 or inl > cands[best][1]:
            best = j
    return best


def _off_integer(v, what):
    v = np.asarray(v, np.float64)
    v = v[np.isfinite(v)]
    if v.size:
        d = np.abs(v - np.rint(v))
        assert d.min() > GUARD, "%s lies within %g of an integer" % (what, GUARD)


def frame_samples(f, *, min_inliers, min_hits, flat, model, thr, train_page, page_xy, pages, guard=True):
    """-> None (the frame does not contribute) or (fv uint8 [n, 3], pv uint8 [n, 3], box (bx0, by0, bx1, by1), hits, page)."""
    slot = contributor(f["cands"], min_inliers)
    if slot < 0:
        return None
    p, _, M = f["cands"][slot]
    p = int(p)
    M = [np.float64(v) for v in M]
    thr2 = np.float64(thr) * np.float64(thr)
    xy = np.asarray(f["xy"], np.float32).reshape(-1, 2)
    hx, hy = [], []
    for q, t in f["votes"]:
        if int(train_page[t]) != p:
            continue
        with np.errstate(all="ignore"):
            d2 = E.residual2(M, model, page_xy[t][0], page_xy[t][1], xy[q][0], xy[q][1])
        if d2 is None or not np.isfinite(d2):
            continue
        if guard:
            assert abs(d2 - thr2) > GUARD * thr2, "a tested pair lies within %g of the threshold: %r vs %r" % (GUARD, d2, thr2)
        if d2 <= thr2:
            hx.append(np.float64(page_xy[t][0])); hy.append(np.float64(page_xy[t][1]))
    if len(hx) < min_hits:
        return None
    bx0, bx1 = int(np.floor(min(hx))), int(np.ceil(max(hx)))
    by0, by1 = int(np.floor(min(hy))), int(np.ceil(max(hy)))
    w, h, small = pages[p]
    small = np.asarray(small, np.uint8)
    sh, sw = small.shape[:2]
    x = ((np.arange(sw, dtype=np.float64) + 0.5) * np.float64(w)) / np.float64(sw) - 0.5
    y = ((np.arange(sh, dtype=np.float64) + 0.5) * np.float64(h)) / np.float64(sh) - 0.5
    if guard:
        _off_integer(x, "a box comparison (x)"); _off_integer(y, "a box comparison (y)")
    inx, iny = (x >= bx0) & (x <= bx1), (y >= by0) & (y <= by1)
    xx, yy = np.meshgrid(x, y)
    with np.errstate(all="ignore"):
        X = M[0] * xx + M[1] * yy + M[2]
        Y = M[3] * xx + M[4] * yy + M[5]
        ok = iny[:, None] & inx[None, :]
        if model == 1:
            wq = M[6] * xx + M[7] * yy + M[8]
            ok &= wq != 0
            X, Y = X / wq, Y / wq
        Xh, Yh = X + 0.5, Y + 0.5
        if guard:
            _off_integer(Xh[ok], "X + 0.5"); _off_integer(Yh[ok], "Y + 0.5")
        Xi, Yi = np.floor(Xh), np.floor(Yh)
        img = np.asarray(f["image"], np.uint8)
        ah, aw = img.shape[:2]
        ok &= (Xi >= 0) & (Xi < aw) & (Yi >= 0) & (Yi < ah)          # (a NaN fails every comparison)
    S = small.astype(np.int32)
    Sp = np.pad(S, ((1, 1), (1, 1), (0, 0)), mode="edge")
    d = np.zeros((sh, sw), np.int32)
    for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
        d = np.maximum(d, np.abs(Sp[dy:dy + sh, dx:dx + sw] - S).max(axis=2))
    ok &= d <= flat
    fv = img[Yi[ok].astype(np.int64), Xi[ok].astype(np.int64)]
    return fv.reshape(-1, 3), small[ok].reshape(-1, 3), (bx0, by0, bx1, by1), len(hx), p


def counts(frames, *, min_inliers, min_hits, flat, model, thr, train_page, page_xy, pages, guard=True, stats=None):
    """-> (cnt uint64 [3, 256], sum uint64 [3, 256], frames_through, frames_counted).  stats: a list that receives, per frame, None or
    (samples, box, hits, page)."""
    assert min_inliers >= 0 and min_hits >= 1 and 0 <= flat <= 255
    cnt, sm = np.zeros((3, 256), np.uint64), np.zeros((3, 256), np.uint64)
    through = counted = 0
    for f in frames:
        through += 1
        r = frame_samples(f, min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=model, thr=thr, train_page=train_page,
                          page_xy=page_xy, pages=pages, guard=guard)
        if stats is not None:
            stats.append(None if r is None else (len(r[0]),) + r[2:])
        if r is None:
            continue
        counted += 1
        fv, pv = r[0], r[1]
        for c in range(3):
            cnt[c] += np.bincount(fv[:, c], minlength=256).astype(np.uint64)
            sm[c] += np.bincount(fv[:, c], weights=pv[:, c].astype(np.float64), minlength=256).astype(np.uint64)      # (< 2^53: exact)
    assert through <= MAX_FRAMES
    return cnt, sm, through, counted


def lut(cnt, sm, min_count):
    """slideo_tone_lut in Python integers -> uint8 [3, 256], or None: a channel without an anchor."""
    assert min_count >= 1
    out = np.zeros((3, 256), np.uint8)
    for c in range(3):
        n = [int(v) for v in cnt[c]]
        s = [int(v) for v in sm[c]]
        anchors = [v for v in range(256) if n[v] >= min_count]
        if not anchors:
            return None
        m, top = {}, 0
        for v in anchors:
            top = max(top, (2 * s[v] + n[v]) // (2 * n[v]))
            m[v] = top
        for x in range(256):
            if x <= anchors[0]:
                out[c, x] = m[anchors[0]]
            elif x >= anchors[-1]:
                out[c, x] = m[anchors[-1]]
            elif x in m:
                out[c, x] = m[x]
            else:
                a = max(v for v in anchors if v < x); b = min(v for v in anchors if v > x)
                out[c, x] = (2 * (m[a] * (b - x) + m[b] * (x - a)) + (b - a)) // (2 * (b - a))
    return out


def frame_record(cfg, xy, desc, cands, train, image, rows=None, votes=None):
    """A frame of `counts` from its features, its candidate records (either implementation's trace, slot order) and its analysed image.
    votes: the frame's votes where the caller has them already (evidence_ref.votes_of otherwise)."""
    return dict(xy=np.asarray(xy, np.float32).reshape(-1, 2), votes=E.votes_of(cfg, desc, train, rows) if votes is None else votes,
                cands=[(int(c["page_idx"]), int(c["inliers"]), np.array(c["transform"], np.float64)) for c in cands],
                image=np.asarray(image, np.uint8))


# ---- the constructed cases both test files use (tests/verify_cases.py builders) ----------------------------------------------------

def black_case():
    """A black frame with 60 exact votes for one page: the picture test fails (no verdict), the candidate has its model."""
    import verify_cases as VC
    c = VC.Case("BLACK", 73)
    c.candidate(c.frame(None), 60, img=0)
    return c


def out_case():
    """One page whose planted map is moved 70 px right and 45 px down: a third of the keypoints, all exact, lie outside the 640x360
    frame (a caller's features may hold any float), so the hit box's image leaves the frame at the right and the bottom."""
    import verify_cases as VC
    c = VC.Case("OUT", 74)
    c.H = c.H.copy(); c.H[0, 2] += 70.0; c.H[1, 2] += 45.0
    c.candidate(c.frame(0), 120, img=0)
    return c


SIZES_B = (600, 338)        # the second page size of sizes_case


def sizes_case():
    """Two pages of different sizes: page 0 the usual 800x450, page 1 600x338 (the top left part of page image 1), a frame for each."""
    import verify_cases as VC
    c = VC.Case("SIZES", 75)
    c.candidate(c.frame(0), 80, img=0)
    pg = c.page(1, filler=0)
    rng = np.random.default_rng(750)
    gx, gy = np.meshgrid(np.arange(45, SIZES_B[0] - 40, 37.0), np.arange(43, SIZES_B[1] - 40, 31.0))
    xy = (np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-3, 3, (gx.size, 2))).astype(np.float32)
    c.link(c.frame(1), pg, c.points(pg, len(xy), xy=xy))
    c.page_sizes = {pg: SIZES_B}
    return c


def page_size(case, i):
    import verify_cases as VC
    return getattr(case, "page_sizes", {}).get(i, (VC.PAGE_W, VC.PAGE_H))


def page_pixels(case, i):
    """The image a page's small image is made of: its page image, cut to the page's size."""
    import verify_cases as VC
    w, h = page_size(case, i)
    return np.ascontiguousarray(VC.page_image(case.pages[i].img)[:h, :w])


def constructed_cases():
    """[(name, (case builder, arguments), page set or None, min_inliers, min_hits, flats)].  verify_model 0 (R2: six candidates, the
    most inliers in the last slot) and 1 (H1), the ratio test, a frame whose most-inlier slot is not its verdict's page (D2 under rule
    0), a frame without a verdict that has a contributor (BLACK), frames below min_inliers (T2: 21 inliers at 22) and below min_hits
    (T2 at 1000 hits), a transform that maps part of the box outside the frame (OUT), flat 0, 2, 8 and 255, a page set (V5 under deck
    pages 0, 7, 16), an empty frame among others (V1), two pages of different sizes (SIZES).  Every hit box clips its page: no
    constructed keypoint lies within 40 px of a page's edge."""
    import verify_cases as VC
    return [("R2", (VC.r2, (10,)), None, 0, 1, (255,)), ("H1", (VC.h1, (1,)), None, 0, 1, (255, 8)), ("RATIO", (E.ratio_case, ()), None, 0, 1, (255,)),
            ("D2-other", (VC.d2, (0,)), None, 0, 1, (0, 2, 8, 255)), ("BLACK", (black_case, ()), None, 0, 1, (255,)),
            ("T2-inliers", (VC.t2, ("rating",)), None, 22, 1, (255,)), ("T2-hits", (VC.t2, ("rating",)), None, 0, 1000, (255,)),
            ("OUT", (out_case, ()), None, 0, 1, (255, 8)), ("V5-set", (VC.v5, (17,)), [0, 7, 16], 0, 1, (255,)),
            ("V1-empty", (VC.v1, ()), None, 0, 1, (255,)), ("SIZES", (sizes_case, ()), None, 0, 20, (255, 0))]


# ---- the darkened canvas scene of "the use" (both test files) ------------------------------------------------------------------------
USE = dict(min_inliers=20, min_hits=20, flat=255, min_count=64, min_rating=12.0)


def darken(frames):
    """The window of the canvas scene (evidence_ref.canvas_scene) darkened as a projector would, the surroundings left alone."""
    g = np.array([0.30, 0.33, 0.27]); o = np.array([38.0, 30.0, 34.0])
    out = np.array(frames, np.uint8, copy=True)
    win = (slice(None), slice(E.WIN_Y, E.WIN_Y + E.WIN_H), slice(E.WIN_X, E.WIN_X + E.WIN_W))
    x = frames[win].astype(np.float64) / 255.0
    out[win] = np.clip(255.0 * g * (x ** 1.3) + o + 0.5, 0, 255).astype(np.uint8)
    return out
