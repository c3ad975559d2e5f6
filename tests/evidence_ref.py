"""The match evidence map (include/slideo_amd.h "Match evidence map") restated in numpy, written from the header: the counts of a
batch of frames from their keypoints, their votes, their verdicts and the winning candidates' transforms, in float64; the mask and
the box made of count arrays.  Nothing here calls the library.

A frame is a dict: xy float32 [K, 2] (the keypoints), votes [(q, t)] (query in frame, train row: every vote of the frame, any
order), page and inliers (its verdict), cands {page: transform (9 values)} (the trace's candidates)."""
import numpy as np

import verify_ref as R

MAX_FRAMES = 1 << 20
GUARD = 1e-9          # no tested pair may lie within this, relative, of the threshold: a condition on the INPUTS


def grid(aw, ah, cell):
    return -(-aw // cell), -(-ah // cell)


def residual2(M, model, x, y, X, Y):
    """dx * dx + dy * dy of the header, each operation rounded once in float64; None: w == 0."""
    M = [np.float64(v) for v in M]
    x, y, X, Y = np.float64(x), np.float64(y), np.float64(X), np.float64(Y)
    px = M[0] * x + M[1] * y + M[2]
    py = M[3] * x + M[4] * y + M[5]
    if model == 1:
        w = M[6] * x + M[7] * y + M[8]
        if w == 0:
            return None
        px, py = px / w, py / w
    dx, dy = px - X, py - Y
    return dx * dx + dy * dy


def counts(frames, *, cell, aw, ah, min_inliers, model, thr, train_page, page_xy, guard=True):
    """-> (seen uint32 [gh, gw], hit uint32 [gh, gw], frames_through, frames_counted)."""
    assert cell in (16, 32, 64)
    gw, gh = grid(aw, ah, cell)
    seen, hit = np.zeros((gh, gw), np.uint32), np.zeros((gh, gw), np.uint32)
    thr2 = np.float64(thr) * np.float64(thr)
    through = counted = 0
    for f in frames:
        through += 1
        if f["page"] < 0 or f["inliers"] < min_inliers:
            continue
        counted += 1
        p = int(f["page"])
        M = f["cands"][p]
        xy = np.asarray(f["xy"], np.float32).reshape(-1, 2)
        is_hit = np.zeros(len(xy), bool)
        for q, t in f["votes"]:
            if int(train_page[t]) != p:
                continue
            with np.errstate(all="ignore"):
                d2 = residual2(M, model, page_xy[t][0], page_xy[t][1], xy[q][0], xy[q][1])
            if d2 is None or not np.isfinite(d2):
                continue
            if guard:
                assert abs(d2 - thr2) > GUARD * thr2, "a tested pair lies within %g of the threshold: %r vs %r" % (GUARD, d2, thr2)
            if d2 <= thr2:
                is_hit[q] = True
        for q, (X, Y) in enumerate(xy):
            if not (X >= 0 and X < aw and Y >= 0 and Y < ah):
                continue
            cx, cy = int(X) // cell, int(Y) // cell
            seen[cy, cx] += 1
            hit[cy, cx] += is_hit[q]
    assert counted <= MAX_FRAMES
    return seen, hit, through, counted


def votes_of(cfg, desc, train, rows=None):
    """Every vote (q, t) of one frame's descriptors against the deck's rows (rows: the train rows a page set searches, ascending)."""
    if len(desc) == 0:
        return []
    sub = train if rows is None else train[rows]
    idx, dist = R.knn(desc, sub, cfg.knn_k)
    v = R.vote(cfg, idx, dist)
    return v if rows is None else [(q, int(rows[t])) for q, t in v]


def frame_record(cfg, xy, desc, verdict, cands, train, rows=None):
    """A frame of `counts` from its features, its verdict record and its candidate records (either implementation's trace)."""
    return dict(xy=np.asarray(xy, np.float32).reshape(-1, 2), votes=votes_of(cfg, desc, train, rows), page=int(verdict["page_idx"]),
                inliers=int(verdict["inliers"]), cands={int(c["page_idx"]): np.array(c["transform"], np.float64) for c in cands})


def deck_of(db, n_pages):
    """-> train_page [M], page_xy [M, 2] f32 of a finalized deck (a Matcher's or the restatement's PageDB: page_features)."""
    tp, xy = [], []
    for p in range(n_pages):
        kp, _ = db.page_features(p)
        tp.append(np.full(len(kp), p, np.int64)); xy.append(np.stack([kp["x"], kp["y"]], 1).astype(np.float32).reshape(-1, 2))
    return np.concatenate(tp), np.concatenate(xy)


def mask(seen, hit, cell, aw, ah, min_seen, min_hit_ppm, grow):
    seen, hit = np.asarray(seen, np.uint64), np.asarray(hit, np.uint64)
    gh, gw = seen.shape
    assert (gw, gh) == grid(aw, ah, cell)
    clutter = (seen >= np.uint64(min_seen)) & (hit * np.uint64(1000000) < np.uint64(min_hit_ppm) * seen)
    keep = ~clutter
    grown = np.zeros_like(keep)
    for y in range(gh):
        for x in range(gw):
            grown[y, x] = keep[max(0, y - grow):y + grow + 1, max(0, x - grow):x + grow + 1].any()
    ys, xs = np.arange(ah) // cell, np.arange(aw) // cell
    return np.where(grown[ys][:, xs], 255, 0).astype(np.uint8)


def box(seen, hit, cell, aw, ah, min_hits, min_hit_ppm):
    seen, hit = np.asarray(seen, np.uint64), np.asarray(hit, np.uint64)
    ok = (hit >= np.uint64(min_hits)) & (hit * np.uint64(1000000) >= np.uint64(min_hit_ppm) * seen)
    if not ok.any():
        return (-1, -1, -1, -1)
    ys, xs = np.nonzero(ok)
    return (int(xs.min()) * cell, int(ys.min()) * cell, min((int(xs.max()) + 1) * cell, aw), min((int(ys.max()) + 1) * cell, ah))


# ---- the constructed cases both test files use (tests/verify_cases.py builders) ----------------------------------------------------

def constructed_cases():
    """[(name, (case builder, arguments), page set or None, min_inliers)]: verify_model 0 and 1, the ratio test, a keypoint with two
    votes for the winner of which one passes (MULTI), frames without a verdict (X1: no model; V1's empty frame, the empty-frame
    case too), a frame below min_inliers (T2: 21 inliers at min_inliers 22), a page set (V5 under deck pages 0, 7, 16)."""
    import verify_cases as VC
    return [("R2", (VC.r2, (10,)), None, 0), ("R3", (VC.r3, (3.0,)), None, 0), ("H1", (VC.h1, (1,)), None, 0),
            ("RATIO", (ratio_case, ()), None, 0), ("V1-empty", (VC.v1, ()), None, 0), ("X1-none", (VC.x1, ()), None, 0),
            ("T2-below", (VC.t2, ("rating",)), None, 22), ("V5-set", (VC.v5, (17,)), [0, 7, 16], 0), ("MULTI", (multi_vote_case, ()), None, 0)]


def ratio_case():
    """The ratio test (0.8) in place of the tolerance vote: one page, 60 votes of which 48 are exact and 12 far outliers."""
    import verify_cases as VC
    c = VC.Case("RATIO", 72, cfg={"ratio_test": 0.8})
    c.candidate(c.frame(0), 60, 0.8, img=0)
    return c


def multi_vote_case():
    """One page whose rows come in pairs of EQUAL descriptors at different points: every frame keypoint votes for both rows of its
    pair (equal distances), both votes go to the winner, and only the vote to the row the keypoint is the image of passes."""
    import verify_cases as VC
    c = VC.Case("MULTI", 71)
    pg = c.page(0, filler=0)
    rows = c.points(pg, 40)
    # the twins: the same descriptors at points 60 px and more away from the first ones' (far outside the threshold)
    twin_xy = c.pages[pg].xy[rows] + np.float32([60.0, 45.0])
    twin_xy[:, 0] = np.where(twin_xy[:, 0] > VC.PAGE_W - 40, twin_xy[:, 0] - 120.0, twin_xy[:, 0])
    twin_xy[:, 1] = np.where(twin_xy[:, 1] > VC.PAGE_H - 40, twin_xy[:, 1] - 90.0, twin_xy[:, 1])
    c.points(pg, 40, xy=twin_xy, desc=c.pages[pg].desc[rows])
    f = c.frame(0)
    c.link(f, pg, rows)
    return c


# ---- the canvas scene of "the use" (both test files) --------------------------------------------------------------------------------
# A 640x360 window at (WIN_X, WIN_Y) in a 960x540 canvas of static random texture.  The window shows the inner 640x360 of a 960x540
# synth frame, whose slide (85 .. 100 % of the frame's width, at most 5 % off centre) always covers that inner part: the slide's
# content runs past the window's edges, as a slide does in a cropped capture, so keypoints agree with their page right up to where a
# descriptor's patch reaches the texture.  At cell 64 the offsets leave 32 pixels of window in the left and right edge cells, 52 in
# the top and bottom ones.  The pages are rows of synth-like glyphs from edge to edge.
CANVAS_W, CANVAS_H, WIN_W, WIN_H, WIN_X, WIN_Y = 960, 540, 640, 360, 160, 76
PAGE_W, PAGE_H = 1600, 900
SCENE = dict(cell=64, min_inliers=20, min_seen=8, min_hit=0.02, min_hits=2, box_min_hit=0.0, grow=0, n_pages=4, n_frames=16, nfeatures=3000)


def canvas_scene(synth):
    """-> (pages, frames uint8 [n, 540, 960, 3], truth)."""
    rng = np.random.default_rng(2028)

    def glyphs(img, c, pitch, margin):                              # rows of 3 x 5-cell glyphs of c pixels, dark on the image's tone
        h, w = img.shape[:2]
        for y in range(margin, h - margin - 5 * c + 1, pitch):
            x = margin
            while x <= w - margin - 3 * c:
                bits = rng.integers(0, 2, (5, 3)).astype(bool)
                bits[rng.integers(0, 5), rng.integers(0, 3)] = True
                on = np.repeat(np.repeat(bits, c, 0), c, 1)
                img[y:y + 5 * c, x:x + 3 * c][on] = rng.integers(0, 80)
                x += 3 * c + int(rng.integers(2 * c, 7 * c))

    pages = np.full((SCENE["n_pages"], PAGE_H, PAGE_W, 3), 255, np.uint8)
    for pg in pages:
        glyphs(pg, 6, 70, 16)
    whole, truth, _ = synth.frames(pages, 2 * SCENE["n_frames"], CANVAS_W, CANVAS_H)
    keep = np.nonzero(np.asarray(truth) >= 0)[0][:SCENE["n_frames"]]          # (a frame without a slide shows nothing to learn from)
    whole, truth = whole[keep], np.asarray(truth)[keep]
    oy, ox = (CANVAS_H - WIN_H) // 2, (CANVAS_W - WIN_W) // 2
    # the texture: 12-pixel blocks of random light tones under random dark marks, the same in every frame
    b = 12
    blocks = rng.integers(150, 256, (-(-CANVAS_H // b), -(-CANVAS_W // b), 3), dtype=np.uint8)
    tex = np.repeat(np.repeat(blocks, b, 0), b, 1)[:CANVAS_H, :CANVAS_W].copy()
    glyphs(tex, 3, 30, 4)
    frames = np.repeat(tex[None], len(whole), 0).copy()
    frames[:, WIN_Y:WIN_Y + WIN_H, WIN_X:WIN_X + WIN_W] = whole[:, oy:oy + WIN_H, ox:ox + WIN_W]
    return pages, frames, truth


def check_use(seen, hit, cell, min_seen, learnt_box, learnt_mask):
    """The box and mask conditions of "the use" on the canvas scene -> (clutter cells zeroed, clutter cells)."""
    x0, y0, x1, y1 = learnt_box
    assert x0 <= WIN_X and y0 <= WIN_Y and x1 >= WIN_X + WIN_W and y1 >= WIN_Y + WIN_H, ("the box misses part of the window", learnt_box)
    assert WIN_X - x0 < cell and WIN_Y - y0 < cell and x1 - (WIN_X + WIN_W) < cell and y1 - (WIN_Y + WIN_H) < cell, ("the box exceeds the window", learnt_box)
    gh, gw = seen.shape
    outside = zeroed = 0
    for cy in range(gh):
        for cx in range(gw):
            cx0, cy0, cx1, cy1 = cx * cell, cy * cell, min((cx + 1) * cell, CANVAS_W), min((cy + 1) * cell, CANVAS_H)
            m = learnt_mask[cy0:cy1, cx0:cx1]
            if cx0 >= WIN_X and cy0 >= WIN_Y and cx1 <= WIN_X + WIN_W and cy1 <= WIN_Y + WIN_H:
                assert (m == 255).all(), ("a cell wholly inside the window is masked", cx, cy)
            elif (cx1 <= WIN_X or cx0 >= WIN_X + WIN_W or cy1 <= WIN_Y or cy0 >= WIN_Y + WIN_H) and seen[cy, cx] >= min_seen:
                outside += 1
                zeroed += int((m == 0).all())
    assert outside > 0 and 2 * zeroed >= outside, ("clutter cells zeroed", zeroed, outside)
    return zeroed, outside
