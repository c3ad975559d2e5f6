"""Constructed feature sets for the verify stage (vote, RANSAC, rating, verdict): small deterministic decks and frames whose
keypoints and descriptors are MADE, not detected, so that every case reaches one branch on purpose.  They go in through
Matcher.add_page_features / Matcher.match_features and PageDB.add_page_features / PageDB.match_features_trace; the expected
values come from tests/verify_ref.py.

Descriptors: a correspondence is a random 256-bit row and the same row with exactly b chosen bits flipped (Hamming distance
exactly b); unrelated rows are random (128 +- 8 apart).  Geometry: page keypoints uniform in an 800x450 page at >= 4 px spacing,
frame keypoints their image under the planted map (model 0: scale 0.8, rotation 3 degrees about the centres; model 1: the same
with a mild projective row), rounded to f32; outliers displaced by 50 px and more, band points by a chosen vector.  Images: smooth
random pages, frames the planted nearest-neighbour warp of the page they show.

Every case is built from np.random.default_rng(seed) alone; check_guards(case) states what every construction must satisfy."""
import numpy as np

PAGE_W, PAGE_H, FRAME_W, FRAME_H = 800, 450, 640, 360
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
N_IMAGES = 4
B_CORR = 3          # Hamming distance of an ordinary correspondence: lim = 3 * 1.05f = 3.15, only the partner votes


def planted_map(model):
    s, a = 0.8, np.deg2rad(3.0)
    c, sn = s * np.cos(a), s * np.sin(a)
    px, py, fx, fy = PAGE_W / 2, PAGE_H / 2, FRAME_W / 2, FRAME_H / 2
    H = np.array([[c, -sn, fx - (c * px - sn * py)], [sn, c, fy - (sn * px + c * py)], [0, 0, 1]], np.float64)
    if model == 1:
        H[2] = [4e-5, -3e-5, 1]
    return H


def apply_map(H, xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    w = H[2, 0] * xy[:, 0] + H[2, 1] * xy[:, 1] + H[2, 2]
    return np.stack([(H[0, 0] * xy[:, 0] + H[0, 1] * xy[:, 1] + H[0, 2]) / w,
                     (H[1, 0] * xy[:, 0] + H[1, 1] * xy[:, 1] + H[1, 2]) / w], 1)


_images = {}


def page_image(i):
    """Smooth random 800x450 BGR page number i: a coarse random grid, bilinearly enlarged."""
    if i not in _images:
        rng = np.random.default_rng(1000 + i)
        gh, gw = 10, 17
        g = rng.uniform(0, 255, (gh, gw, 3))
        y = np.linspace(0, gh - 1, PAGE_H); x = np.linspace(0, gw - 1, PAGE_W)
        y0 = np.minimum(y.astype(int), gh - 2); x0 = np.minimum(x.astype(int), gw - 2)
        fy = (y - y0)[:, None, None]; fx = (x - x0)[None, :, None]
        a = g[y0][:, x0]; b = g[y0][:, x0 + 1]; c = g[y0 + 1][:, x0]; d = g[y0 + 1][:, x0 + 1]
        _images[i] = np.rint((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy).astype(np.uint8)
    return _images[i]


_frames = {}


def frame_image(i, model):
    """The 640x360 frame that shows page image i under the planted map (nearest neighbour, black outside)."""
    if (i, model) not in _frames:
        Hi = np.linalg.inv(planted_map(model))
        X, Y = np.meshgrid(np.arange(FRAME_W, dtype=np.float64), np.arange(FRAME_H, dtype=np.float64))
        p = apply_map(Hi, np.stack([X.ravel(), Y.ravel()], 1))
        sx = np.rint(p[:, 0]).astype(int); sy = np.rint(p[:, 1]).astype(int)
        ok = (sx >= 0) & (sx < PAGE_W) & (sy >= 0) & (sy < PAGE_H)
        out = np.zeros((FRAME_H * FRAME_W, 3), np.uint8)
        out[ok] = page_image(i)[sy[ok], sx[ok]]
        _frames[(i, model)] = out.reshape(FRAME_H, FRAME_W, 3)
    return _frames[(i, model)]


def keypoints(xy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    kp = np.zeros(len(xy), KEYPOINT_DTYPE)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]; kp["size"] = 31.0; kp["response"] = 1.0
    return kp


class Page:
    def __init__(self, img):
        self.img = img
        self.xy = np.zeros((0, 2), np.float32)
        self.desc = np.zeros((0, 32), np.uint8)


class Frame:
    def __init__(self, img):
        self.img = img                       # page image shown (None: black frame)
        self.xy = np.zeros((0, 2), np.float32)
        self.desc = np.zeros((0, 32), np.uint8)
        self.partner = []                    # per query: the set of train (page, row) it is meant to be near
        self.band = []                       # per query: a band point (placed at a stated distance from the threshold)
        self.inlier = []                     # per query: what the planted set says of its vote
        self.planted = {}                    # page -> per vote, in vote order: True (planted inlier) / False
        self.exact = {}                      # page -> per vote: True where the point is the planted image itself (no displacement)


class Case:
    def __init__(self, name, seed, model=0, cfg=None, envs=None):
        self.name, self.model = name, model
        self.cfg = dict(cfg or {})           # overrides on small_cfg
        if model == 1:
            self.cfg.setdefault("verify_model", 1)
        self.envs = envs or [{}]             # environment variants of the GPU library: identical records expected under each
        self.rng = np.random.default_rng(seed)
        self.H = planted_map(model)
        self.pages, self.frames = [], []
        self.expect = {}                     # what the case states beyond "equals verify_ref" (used by the tests)

    # ---- construction ---------------------------------------------------------------------------------------------------------
    def rows(self, n):
        return self.rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def flipped(self, rows, b):
        """Each row with exactly b chosen bits flipped."""
        out = np.array(rows, np.uint8, copy=True).reshape(-1, 32)
        for r in out:
            for bit in self.rng.choice(256, b, replace=False):
                r[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return out

    def page(self, img=None, filler=1):
        """A new page with `filler` unrelated keypoints -> its index."""
        p = Page(len(self.pages) % N_IMAGES if img is None else img)
        self.pages.append(p)
        if filler:
            self.points(len(self.pages) - 1, filler)
        return len(self.pages) - 1

    def points(self, page, n, xy=None, desc=None):
        """n more keypoints on a page (uniform at >= 4 px spacing inside the margin that the planted map keeps in the frame, or
        the given coordinates) with fresh random rows (or the given ones) -> their row numbers on the page."""
        p = self.pages[page]
        if xy is None:
            got = np.zeros((0, 2), np.float32)
            while len(got) < n:
                c = np.stack([self.rng.uniform(40, PAGE_W - 40, 4 * n + 16), self.rng.uniform(40, PAGE_H - 40, 4 * n + 16)], 1).astype(np.float32)
                for q in c:
                    ref = np.concatenate([p.xy, got])
                    if len(ref) == 0 or ((ref - q) ** 2).sum(1).min() >= 16.0:
                        got = np.concatenate([got, q[None]])
                        if len(got) == n:
                            break
            xy = got
        xy = np.asarray(xy, np.float32).reshape(-1, 2)
        first = len(p.xy)
        p.xy = np.concatenate([p.xy, xy])
        p.desc = np.concatenate([p.desc, self.rows(len(xy)) if desc is None else np.asarray(desc, np.uint8).reshape(-1, 32)])
        return list(range(first, first + len(xy)))

    def frame(self, img=None):
        self.frames.append(Frame(img))
        return len(self.frames) - 1

    def link(self, frame, page, rows, b=B_CORR, disp=None, inlier=True, also=(), band=False):
        """One frame keypoint per page row in `rows`: descriptor = the page row with b bits flipped, position = the planted image
        of the page point plus disp (one vector, or one per row; None: exact).  also: further (page, row) holding the SAME
        descriptor and point (duplicate rows).  inlier: what the planted set says of these votes."""
        f, p = self.frames[frame], self.pages[page]
        rows = list(rows)
        to = apply_map(self.H, p.xy[rows])
        if disp is not None:
            to = to + np.asarray(disp, np.float64).reshape(-1, 2)
        f.xy = np.concatenate([f.xy, to.astype(np.float32)])
        f.desc = np.concatenate([f.desc, self.flipped(p.desc[rows], b)])
        for r in rows:
            f.partner.append({(page, r)} | {(pp, rr[rows.index(r)]) for pp, rr in also})
            f.band.append(band); f.inlier.append(bool(inlier))
        for pg in [page] + [pp for pp, _ in also]:
            f.planted.setdefault(pg, []).extend([bool(inlier)] * len(rows))
            f.exact.setdefault(pg, []).extend([disp is None] * len(rows))

    def far(self, n):
        """n outlier displacements of 50 .. 150 px in random directions."""
        a = self.rng.uniform(0, 2 * np.pi, n); r = self.rng.uniform(50, 150, n)
        return np.stack([r * np.cos(a), r * np.sin(a)], 1)

    def candidate(self, frame, n, inlier_frac=1.0, page=None, img=None):
        """A page (new unless given) with n fresh points, all voted for by the frame: round(n * frac) of them exact, the rest far
        outliers, the two kinds mixed at random along the query order -> the page."""
        if page is None:
            page = self.page(img)
        rows = self.points(page, n)
        n_in = int(round(n * inlier_frac))
        order = self.rng.permutation(n)
        disp = np.zeros((n, 2)); far = self.far(n - n_in)
        is_in = np.zeros(n, bool)
        is_in[order[:n_in]] = True
        disp[~is_in] = far
        for i in range(n):
            self.link(frame, page, [rows[i]], disp=None if is_in[i] else disp[i], inlier=bool(is_in[i]))
        return page

    # ---- what the implementations take ----------------------------------------------------------------------------------------
    def deck(self):
        """-> train [M, 32], train_page [M], page_xy [M, 2]: the rows in page order."""
        train = np.concatenate([p.desc for p in self.pages])
        tp = np.concatenate([np.full(len(p.xy), i, np.int64) for i, p in enumerate(self.pages)])
        xy = np.concatenate([p.xy for p in self.pages])
        return train, tp, xy

    def frame_pixels(self, i):
        f = self.frames[i]
        return np.zeros((FRAME_H, FRAME_W, 3), np.uint8) if f.img is None else frame_image(f.img, self.model)


def check_guards(case, thr):
    """What every construction satisfies: (1) no unintended (query, train row) pair is nearer than 65; (2) under the planted map no
    vote's residual lies within 0.05 px of the threshold (R3's band points: at their stated distances) and every outlier is at
    least 50 px away; (3) page points are >= 4 px apart unless the case asked for a coincidence (expect["coincident"]); (4) exact
    frame points lie inside the frame."""
    import verify_ref as R
    train, tp, _ = case.deck()
    ofs = np.concatenate([[0], np.cumsum([len(p.xy) for p in case.pages])])
    for f in case.frames:
        if len(f.desc) == 0:
            continue
        d = R.hamming(f.desc, train)
        for q, partners in enumerate(f.partner):
            for pg, r in partners:
                d[q, ofs[pg] + r] = 999
        assert d.min() > 64, d.min()
        for q, partners in enumerate(f.partner):
            for pg, r in partners:
                if pg not in f.planted:          # (a hand-made neighbour list: single votes, no geometry)
                    continue
                res = np.linalg.norm(apply_map(case.H, case.pages[pg].xy[r])[0] - f.xy[q].astype(np.float64))
                # (R3's band points sit at their stated distances: 0.1 px and more from the threshold 3, half of it from 1.5)
                assert abs(res - thr) > (0.04 * thr / 3.0 if f.band[q] else 0.05), (case.name, res)
                assert f.inlier[q] or f.band[q] or res >= 50.0 - 1e-3, (case.name, res)
    for i, p in enumerate(case.pages):
        if len(p.xy) > 1 and i not in case.expect.get("coincident", ()):
            d2 = ((p.xy[:, None, :].astype(np.float64) - p.xy[None, :, :]) ** 2).sum(2) + 1e9 * np.eye(len(p.xy))
            assert d2.min() >= 16.0 - 1e-3, (case.name, i, d2.min())
    for f in case.frames:
        if len(f.xy):
            exact = np.zeros(len(f.xy), bool)
            for q, partners in enumerate(f.partner):
                pg, r = sorted(partners)[0]
                res = np.linalg.norm(apply_map(case.H, case.pages[pg].xy[r])[0] - f.xy[q].astype(np.float64))
                exact[q] = res < 1e-3
            e = f.xy[exact]
            assert len(e) == 0 or (e.min() >= 0 and e[:, 0].max() < FRAME_W and e[:, 1].max() < FRAME_H), case.name


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# (min_rating 2: a case whose survivors have few inliers; 2 itself keeps every 2-vote candidate — closed form, NaN on coincident
# points — out of the survivors, as `rating > min_rating` is strict)

def v1():
    """One page; frames with 0 / 1 / 255 / 256 / 257 / 513 keypoints in one call, the empty one in the middle."""
    c = Case("V1", 11)
    pg = c.page(0, filler=0)
    rows = c.points(pg, 513)
    for n in (1, 255, 256, 0, 257, 513):
        f = c.frame(0)
        if n:
            c.link(f, pg, rows[:n])
    return c


def v2():
    """Tolerance edges: neighbours at (20, 20, 21), (40, 41, 42), (19, 19, 20), (0, 0, 1) on distinct pages; d < best * 1.05f votes."""
    c = Case("V2", 12)
    f = c.frame(0)
    want = []
    for dists in ((20, 20, 21), (40, 41, 42), (19, 19, 20), (0, 0, 1)):
        q = c.rows(1)
        pgs = []
        for d in dists:
            pg = c.page()
            r = c.points(pg, 1, desc=c.flipped(q, d))[0]
            pgs.append((pg, r, d))
        lim = np.float32(dists[0]) * np.float32(1.05)
        want += [pg for pg, _, d in pgs if np.float32(d) < lim]
        # the query sits at the planted image of its first partner's point
        pg0, r0, _ = pgs[0]
        fr = c.frames[f]
        fr.xy = np.concatenate([fr.xy, apply_map(c.H, c.pages[pg0].xy[r0]).astype(np.float32)])
        fr.desc = np.concatenate([fr.desc, q])
        fr.partner.append({(pg, r) for pg, r, _ in pgs}); fr.band.append(False); fr.inlier.append(True)
    c.expect["voted_pages"] = sorted(want)
    return c


def v3(mode):
    """Fewer train rows than knn_k (30).  tol: a 3-row deck under the tolerance vote; one: ratio mode with a 1-row deck (no
    vote); r12 / r13: ratio mode (0.8f) with the two rows at distances (10, 12) / (10, 13): 10 < 0.8f * d1 decides."""
    c = Case("V3-" + mode, 13, cfg={} if mode == "tol" else {"ratio_test": 0.8})
    f = c.frame(0)
    pg = c.page(0, filler=0)
    if mode == "tol":
        c.link(f, pg, c.points(pg, 3))
    elif mode == "one":
        c.link(f, pg, c.points(pg, 1))
    else:
        d1 = 12 if mode == "r12" else 13
        q = c.rows(1)
        r = c.points(pg, 1, desc=c.flipped(q, 10))[0]
        pg2 = c.page(1, filler=0)
        r2 = c.points(pg2, 1, desc=c.flipped(q, d1))[0]
        fr = c.frames[f]
        fr.xy = np.concatenate([fr.xy, apply_map(c.H, c.pages[pg].xy[r]).astype(np.float32)])
        fr.desc = np.concatenate([fr.desc, q])
        fr.partner.append({(pg, r), (pg2, r2)}); fr.band.append(False); fr.inlier.append(True)
        c.expect["n_votes"] = int(np.float32(10) < np.float32(0.8) * np.float32(d1))
    return c


def v4(rule=0):
    """Duplicate rows: pages 2 and 5 hold the same 30 descriptors, points and picture; both vote (the search's de-duplication
    restores the twin), tie everywhere, and the verdict goes to page 2.  (D1: under verdict rule 0 and 1.)"""
    c = Case("V4-rule%d" % rule, 14, cfg={"verdict_rule": rule})
    for i in range(6):
        c.page(img=2 if i in (2, 5) else (0 if i < 2 else 1))
    rows2 = c.points(2, 30)
    rows5 = c.points(5, 30, xy=c.pages[2].xy[rows2], desc=c.pages[2].desc[rows2])
    f = c.frame(2)
    c.link(f, 2, rows2, also=[(5, rows5)])
    c.expect["verdict_page"] = 2
    return c


def v5(P, max_cand=40):
    """P pages, most with one unrelated keypoint.  P = 257: 45 pages are voted for; the counts of voted pages 38 .. 44 (in page
    order) tie, so the cut at 40 keeps the lower page indices."""
    c = Case("V5-P%d-c%d" % (P, max_cand), 15, cfg={"max_candidate_pages": max_cand, "min_rating": 2.0})
    for _ in range(P):
        c.page()
    f = c.frame(0)
    if P == 257:
        voted = [3 + 5 * i for i in range(45)]
        counts = [4 + (i * 7) % 5 for i in range(38)] + [3] * 7
    elif P == 17:
        voted, counts = [16, 0, 7], [5, 5, 9]
    else:
        voted, counts = [0], [20]
    for pg, n in zip(voted, counts):
        c.candidate(f, n, page=pg)
    order = sorted(zip(voted, counts), key=lambda t: (-t[1], t[0]))
    c.expect["cand_pages"] = [pg for pg, _ in order][:max_cand]
    return c


def r1():
    """Model 0 small counts on one frame: 1, 2, 2 coincident (NaN model, 2 inliers, never survives), 3, 4, 63, 64, 65 votes."""
    c = Case("R1", 21, cfg={"min_rating": 2.0})
    f = c.frame(0)
    for n in (1, 2):
        c.candidate(f, n)
    pg = c.page()
    xy = np.float32([[401.5, 203.25]])                       # two page keypoints on one point: the closed form divides by zero
    c.link(f, pg, c.points(pg, 2, xy=np.concatenate([xy, xy])))
    c.expect["coincident"] = (pg,)
    for n in (3, 4, 63, 64, 65):
        c.candidate(f, n)
    return c


def r2(refine):
    """The instance seams: 255 / 256 / 257 / 1023 / 1024 / 1025 votes, 60 % inliers, 40 % far outliers."""
    c = Case("R2-refine%d" % refine, 22, cfg={"refine_iters": refine})
    f = c.frame(0)
    for n in (255, 256, 257, 1023, 1024, 1025):
        c.candidate(f, n, 0.6)
    c.expect["planted"] = True
    return c


R3_SEEDS = {3.0: 23, 1.5: 23}


def r3(thr):
    """Threshold band: 200 exact inliers and 20 each displaced by k * (2.9, 0) in, (3.1, 0) out, (2.5, 2.5) out (norm 3.54 k),
    (2.0, 2.0) in (norm 2.83 k), k = thr / 3, in shuffled query order.  (The seed is one under which the estimator's accepted
    sample is a pair of exact points: a sample through a band point can gather the whole band.)"""
    c = Case("R3-thr%g" % thr, R3_SEEDS[thr], cfg={"ransac_threshold": thr})
    k = thr / 3.0
    f = c.frame(0)
    pg = c.page(0)
    rows = c.points(pg, 280)
    kinds = [(None, True)] * 200
    for d, inl in (((2.9, 0), True), ((3.1, 0), False), ((2.5, 2.5), False), ((2.0, 2.0), True)):
        kinds += [((d[0] * k, d[1] * k), inl)] * 20
    for r, j in zip(rows, c.rng.permutation(280)):
        c.link(f, pg, [r], disp=kinds[j][0], inlier=kinds[j][1], band=kinds[j][0] is not None)
    c.expect["planted"] = True
    return c


def r4(max_iters):
    """Early stop and iteration cap: 95 % inliers, confidence 0.9."""
    c = Case("R4-it%d" % max_iters, 24, cfg={"ransac_max_iters": max_iters, "ransac_confidence": 0.9})
    c.candidate(c.frame(0), 100, 0.95, img=0)
    return c


def r5():
    """The redraw schedule from the LDS window and by the prefix-sum fixed point (SLIDEO_RANSAC_WINDOW 1 / 0) on 3 and 5 votes."""
    c = Case("R5", 25, cfg={"min_rating": 2.0}, envs=[{"SLIDEO_RANSAC_WINDOW": "1"}, {"SLIDEO_RANSAC_WINDOW": "0"}])
    f = c.frame(0)
    c.candidate(f, 3)
    c.candidate(f, 5)
    return c


def h1(hdlt):
    """Model 1: 3 votes (not found), 4, 5, 4 with three collinear, 5 on one line, 256 / 257 / 1024 / 1025 at 60 %.
    (Exactly four votes are fitted directly, as cv::findHomography does, without the sample's subset check — which looks only at
    the triples that hold the sample's LAST point; of five votes on one line every sample fails it and nothing is found.)"""
    c = Case("H1-hdlt%d" % hdlt, 31, model=1, cfg={"ocv_hdlt": hdlt, "min_rating": 2.0})
    f = c.frame(0)
    for n in (3, 4, 5):
        c.candidate(f, n)
    pg = c.page(filler=0)
    c.link(f, pg, c.points(pg, 4, xy=np.float32([[100, 100], [200, 150], [300, 200], [150, 300]])))
    c.expect["collinear4"] = pg
    pg = c.page(filler=0)
    c.link(f, pg, c.points(pg, 5, xy=np.float32([[100, 100], [200, 150], [300, 200], [400, 250], [500, 300]])))
    c.expect["collinear5"] = pg
    for n in (256, 257, 1024, 1025):
        c.candidate(f, n, 0.6)
    c.expect["planted"] = True
    return c


def h2(hdlt):
    """The tail kernel: SLIDEO_RH_TAIL_ROUNDS 0 (cap off) and 1 (every sampled candidate handed over) on 257 and 1025 votes."""
    c = Case("H2-hdlt%d" % hdlt, 32, model=1, cfg={"ocv_hdlt": hdlt}, envs=[{"SLIDEO_RH_TAIL_ROUNDS": "0"}, {"SLIDEO_RH_TAIL_ROUNDS": "1"}])
    f = c.frame(0)
    c.candidate(f, 257, 0.6)
    c.candidate(f, 1025, 0.6)
    return c


def h3():
    """The refit's LM in its own wave and in the eigen kernel's lanes (SLIDEO_REFINE_LANE_LM 0 / 1) on 48 and 49 votes."""
    c = Case("H3", 33, model=1, envs=[{"SLIDEO_REFINE_LANE_LM": "0"}, {"SLIDEO_REFINE_LANE_LM": "1"}])
    f = c.frame(0)
    c.candidate(f, 48, 0.75)
    c.candidate(f, 49, 0.75)
    return c


def t1():
    """64 candidates on one frame, max_candidate_pages 64, max_rated 16: the inlier counts of rating ranks 14, 15, 16 tie (16
    inliers), so the cut keeps the two lower candidate slots.  Votes and inliers differ (outliers) so that the rating order is not
    the candidate order."""
    c = Case("T1", 41, cfg={"max_candidate_pages": 64, "max_rated": 16, "min_rating": 2.0})
    f = c.frame(0)
    inl = [30 - i for i in range(14)] + [16, 16, 16] + [3 + i % 6 for i in range(47)]
    out = [(i * 5) % 7 if n >= 16 else 0 for i, n in enumerate(inl)]
    perm = c.rng.permutation(64)
    for j in perm:
        n = inl[j] + out[j]
        c.candidate(f, n, inl[j] / n)
    c.expect["tie_at_cut"] = (16, 16)                # (inlier count of the tie, max_rated)
    return c


def t2(which):
    """rating: min_rating 20 with exactly 20 (out) and 21 (in) inliers; ratio: min_rating_ratio 0.25, best 40, exactly 10 (out)
    and 11 (in); one: max_rated 1."""
    cfg = {"rating": {"min_rating": 20.0, "min_rating_ratio": 0.0}, "ratio": {"min_rating": 5.0, "min_rating_ratio": 0.25},
           "one": {"max_rated": 1, "min_rating": 2.0}}[which]
    c = Case("T2-" + which, 42, cfg=cfg)
    f = c.frame(0)
    counts = {"rating": (21, 20), "ratio": (40, 11, 10), "one": (30, 25, 20)}[which]
    pgs = [c.candidate(f, n) for n in counts]
    c.expect["survivors"] = {"rating": pgs[:1], "ratio": pgs[:2], "one": pgs[:1]}[which]
    return c


def d2(rule):
    """A survivor with more inliers but the worse picture: the frame shows page B's image, page A has 40 inliers, B 25.  Rule 0
    takes B (the best picture), rule 1 takes A (the first accepted in rating order; min_similarity loosened to accept it)."""
    c = Case("D2-rule%d" % rule, 52, cfg={"verdict_rule": rule, "min_similarity": -1.0})
    f = c.frame(1)
    a = c.candidate(f, 40, img=0)
    b = c.candidate(f, 25, img=1)
    c.expect["verdict_page"] = b if rule == 0 else a
    return c


def d3():
    """65 frames in one call (the verdict kernel's 64-frame block seam), all the same single-page case but frame 64: empty."""
    c = Case("D3", 53)
    pg = c.page(0)
    rows = c.points(pg, 30)
    for i in range(65):
        f = c.frame(0)
        if i != 64:
            c.link(f, pg, rows)
            if i:                                   # the same features in every frame
                c.frames[f].desc = c.frames[0].desc
    c.expect["identical_frames"] = True
    return c


def x1():
    """No model at all: 40 votes, every one a far outlier.  RANSAC runs its 2000 iterations (4000 draws and the redraws), which
    is what outruns a short pre-drawn RNG stream (the tap's own growth path)."""
    c = Case("X1", 61)
    c.candidate(c.frame(0), 40, 0.0, img=0)
    return c


def all_cases():
    """The (builder, arguments) of every case (built when asked for: build())."""
    cases = [(v1, ()), (v2, ())] + [(v3, (m,)) for m in ("tol", "one", "r12", "r13")] + [(v4, (0,)), (v4, (1,))]
    cases += [(v5, (1,)), (v5, (17,)), (v5, (257, 40)), (v5, (257, 64)), (v5, (257, 1))]
    cases += [(r1, ()), (r2, (0,)), (r2, (10,)), (r3, (3.0,)), (r3, (1.5,))] + [(r4, (n,)) for n in (1, 37, 64, 65, 2000)] + [(r5, ())]
    cases += [(h1, (h,)) for h in (0, 1, 2)] + [(h2, (h,)) for h in (1, 2)] + [(h3, ())]
    cases += [(t1, ())] + [(t2, (w,)) for w in ("rating", "ratio", "one")] + [(d2, (0,)), (d2, (1,)), (d3, ()), (x1, ())]
    return cases


_built = {}


def build(fn, args):
    key = (fn.__name__, args)
    if key not in _built:
        _built[key] = fn(*args)
    return _built[key]


def case_id(fa):
    fn, args = fa
    return fn.__name__.upper() + ("-" + "-".join(str(a) for a in args) if args else "")


# ---- what a case states beyond "equals verify_ref" ------------------------------------------------------------------------------

def check_expectations(case, fi, pages, n_votes, inliers, survived, verdict_page):
    """The case's own statements on one frame's records (either implementation's)."""
    e = case.expect
    pages = [int(p) for p in pages]
    if "voted_pages" in e:
        assert sorted(pages) == e["voted_pages"] and set(n_votes) == {1}
    if "n_votes" in e:
        assert sum(n_votes) == e["n_votes"]
    if "cand_pages" in e:
        assert pages == e["cand_pages"]
    if "survivors" in e:
        assert [p for p, s in zip(pages, survived) if s] == e["survivors"]
    if "verdict_page" in e:
        assert verdict_page == e["verdict_page"]
    if "coincident" in e:
        i = pages.index(e["coincident"][0])
        assert n_votes[i] == 2 and inliers[i] == 2 and not survived[i]
    if "collinear5" in e:
        i = pages.index(e["collinear5"])
        assert n_votes[i] == 5 and inliers[i] == 0 and not survived[i]
    if "tie_at_cut" in e:
        tie, top = e["tie_at_cut"]
        slots = [i for i, x in enumerate(inliers) if x == tie]
        assert len(slots) == 3 and [int(survived[i]) for i in slots] == [1, 1, 0] and sum(survived) == top
        assert sum(x > tie for x in inliers) == top - 2
    if "planted" in e:
        f = case.frames[fi]
        for pg, nv, inl in zip(pages, n_votes, inliers):
            if pg in f.planted and nv >= 200:
                assert inl == sum(f.planted[pg]), (case.name, pg, inl, sum(f.planted[pg]))


def planted_residual(case, fi, page, M, votes):
    """Max distance, over the votes (queries, page rows) of a candidate that are exact planted inliers, between M's image of the
    page point and the frame point."""
    f, p = case.frames[fi], case.pages[page]
    frm = np.array([p.xy[t] for t in votes[1]], np.float32)
    to = np.array([f.xy[q] for q in votes[0]], np.float32)
    res = np.linalg.norm(apply_map(np.asarray(M, np.float64).reshape(3, 3), frm) - to, axis=1)
    ex = np.array(f.exact[page], bool) & np.array(f.planted[page], bool)
    return float(res[ex].max())


# ---- the definition's answer for a case -----------------------------------------------------------------------------------------

def estimator(oracle, cfg):
    """The restatement's point-level estimator under cfg as verify_ref's estimator(from_xy, to_xy) -> (found, M 3x3, mask)."""
    def est(frm, to):
        if cfg.verify_model == 1:
            found, H, mask, _ = oracle.find_homography(frm, to, cfg)
            return found, (H if found else np.zeros((3, 3))), mask
        found, M, mask, _ = oracle.estimate_affine_partial(frm, to, cfg)
        M3 = np.zeros((3, 3))
        if found:
            M3[:2] = M; M3[2, 2] = 1.0
        return found, M3, mask
    return est


def reference(case, oracle, cfg):
    """verify_ref.stage of every frame of the case (computed once per case)."""
    import verify_ref as R
    if getattr(case, "_ref", None) is None:
        train, tp, pxy = case.deck()
        est = estimator(oracle, cfg)
        case._ref = [R.stage(cfg, train, tp, pxy, f.xy, f.desc, est) for f in case.frames]
    return case._ref
