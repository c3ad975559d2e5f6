"""The match placement map (include/slideo_amd.h "Match placement map") restated in numpy, written from the header: the five sums of a
batch of frames from their keypoints, their votes and their candidate records, in float64 and Python integers; the quad fitted to
sum arrays with numpy.linalg.lstsq.  Nothing here calls the library.

A frame is a dict: xy float32 [K, 2] (the keypoints), votes [(q, t)] (query in frame, train row: every vote of the frame, any
order), cands [(page, inliers, transform (9 values))] in slot order (the trace's candidates).  page_sizes: {page: (pw, ph)}."""
import numpy as np

import evidence_ref as E
import tone_ref as T

MAX_FRAMES = 1 << 20
GUARD = 1e-9          # no tested d2 may lie within this, relative, of reach^2 or of a rival d2: a condition on the INPUTS
TRIM_GUARD = 1e-6     # no cell residual may lie within this many pixels of trim_px


def sums(frames, *, cell, aw, ah, min_inliers, reach, model, train_page, page_xy, page_sizes, guard=True, stats=None):
    """-> (sums uint64 [5, gh, gw]: n, sfx, sfy, su, sv; frames_through, frames_counted).  stats: a dict that receives what the tests
    state about a case: keypoints with several passing votes ("rivals"), with bit-equal best votes ("ties"), page points outside
    their page ("outside"), passing votes ("passing")."""
    assert cell in (16, 32, 64) and min_inliers >= 0 and reach > 0
    gw, gh = E.grid(aw, ah, cell)
    acc = [[[0] * gw for _ in range(gh)] for _ in range(5)]
    reach2 = np.float64(reach) * np.float64(reach)
    through = counted = 0
    st = dict(rivals=0, ties=0, outside=0, passing=0, nearer_is_higher_row=0)
    for f in frames:
        through += 1
        slot = T.contributor(f["cands"], min_inliers)
        if slot < 0:
            continue
        counted += 1
        p, _, M = f["cands"][slot]
        p = int(p)
        pw, ph = page_sizes[p]
        xy = np.asarray(f["xy"], np.float32).reshape(-1, 2)
        best = {}                                                  # q -> [(d2, t)] of its passing votes
        for q, t in f["votes"]:
            if int(train_page[t]) != p:
                continue
            with np.errstate(all="ignore"):
                d2 = E.residual2(M, model, page_xy[t][0], page_xy[t][1], xy[q][0], xy[q][1])
            if d2 is None or not np.isfinite(d2):
                continue
            if guard:
                assert abs(d2 - reach2) > GUARD * reach2, "a tested pair lies within %g of reach^2: %r vs %r" % (GUARD, d2, reach2)
            if d2 <= reach2:
                best.setdefault(int(q), []).append((np.float64(d2), int(t)))
        for q, lst in best.items():
            st["passing"] += len(lst)
            if len(lst) > 1:
                st["rivals"] += 1
                ds = sorted(d for d, _ in lst)
                for a, b in zip(ds, ds[1:]):
                    if a == b:
                        continue                                   # (bit-equal: the row decides)
                    if guard:
                        assert b - a > GUARD * b, "two passing votes of keypoint %d lie within %g of each other: %r %r" % (q, GUARD, a, b)
            dmin = min(d for d, _ in lst)
            rows = sorted(t for d, t in lst if d == dmin)
            st["ties"] += len(rows) > 1
            t = rows[0]
            st["nearer_is_higher_row"] += t != min(tt for _, tt in lst)
            X, Y = xy[q]
            if not (X >= 0 and X < aw and Y >= 0 and Y < ah):
                continue
            x, y = np.float64(page_xy[t][0]), np.float64(page_xy[t][1])
            if pw < 2 or ph < 2 or not (x >= 0 and x <= pw - 1 and y >= 0 and y <= ph - 1):
                st["outside"] += 1
                continue
            cx, cy = int(X) // cell, int(Y) // cell
            add = (1, int(np.rint(np.float64(X) * np.float64(16.0))), int(np.rint(np.float64(Y) * np.float64(16.0))),
                   int(np.rint(x / np.float64(pw - 1) * np.float64(1048576.0))), int(np.rint(y / np.float64(ph - 1) * np.float64(1048576.0))))
            for i in range(5):
                acc[i][cy][cx] += add[i]
    assert through <= MAX_FRAMES
    if stats is not None:
        stats.update(st)
    return np.array(acc, np.uint64).reshape(5, gh, gw), through, counted


def frame_record(cfg, xy, desc, cands, train, rows=None, votes=None):
    """A frame of `sums` from its features and its candidate records (either implementation's trace, slot order)."""
    return dict(xy=np.asarray(xy, np.float32).reshape(-1, 2), votes=E.votes_of(cfg, desc, train, rows) if votes is None else votes,
                cands=[(int(c["page_idx"]), int(c["inliers"]), np.array(c["transform"], np.float64)) for c in cands])


# ---- the quad --------------------------------------------------------------------------------------------------------------------

def points(sm, min_count):
    """-> (cells [(cy, cx)], u, v, X, Y) of the cells with n >= min_count."""
    n = np.asarray(sm[0], np.uint64)
    ys, xs = np.nonzero(n >= np.uint64(min_count))
    k = n[ys, xs].astype(np.float64)
    g = lambda i: np.asarray(sm[i], np.uint64)[ys, xs].astype(np.float64)
    return list(zip(ys.tolist(), xs.tolist())), g(3) / k / 1048576.0, g(4) / k / 1048576.0, g(1) / k / 16.0, g(2) / k / 16.0


def _fit(u, v, X, Y, s):
    xh, yh = X / s, Y / s
    z, o = np.zeros_like(u), np.ones_like(u)
    A = np.concatenate([np.stack([u, v, o, z, z, z, -xh * u, -xh * v], 1), np.stack([z, z, z, u, v, o, -yh * u, -yh * v], 1)])
    b = np.concatenate([xh, yh])
    h, _, rank, _ = np.linalg.lstsq(A, b, rcond=1e-10)
    if rank < 8 or not np.isfinite(h).all():
        return None
    return np.append(h, 1.0).reshape(3, 3)


def apply(H, s, u, v):
    with np.errstate(all="ignore"):
        w = H[2, 0] * u + H[2, 1] * v + 1.0
        return s * ((H[0, 0] * u + H[0, 1] * v + H[0, 2]) / w), s * ((H[1, 0] * u + H[1, 1] * v + H[1, 2]) / w)


def quad(sm, cell, aw, ah, min_count, trim_px, rounds, guard=True):
    """-> None (refused) or (quad float64 [4, 2], H [3, 3], kept cells [(cy, cx)], rms_px)."""
    assert (sm.shape[2], sm.shape[1]) == E.grid(aw, ah, cell) and min_count >= 1 and trim_px > 0 and 0 <= rounds <= 8
    cells, u, v, X, Y = points(sm, min_count)
    s = float(max(aw, ah))
    keep = np.ones(len(cells), bool)
    if keep.sum() < 4:
        return None
    H = _fit(u, v, X, Y, s)
    if H is None:
        return None

    def residuals():
        px, py = apply(H, s, u, v)
        with np.errstate(all="ignore"):
            r = np.sqrt((px - X) ** 2 + (py - Y) ** 2)
        return np.where(np.isfinite(r), r, np.inf)
    for _ in range(rounds):
        r = residuals()
        if guard:
            assert (np.abs(r[keep] - trim_px) > TRIM_GUARD).all(), "a cell residual lies within %g px of trim_px" % TRIM_GUARD
        new = keep & (r <= trim_px)
        if new.sum() == keep.sum():
            break
        keep = new
        if keep.sum() < 4:
            return None
        H = _fit(u[keep], v[keep], X[keep], Y[keep], s)
        if H is None:
            return None
    r = residuals()[keep]
    if not np.isfinite(r).all():
        return None
    q = np.stack(apply(H, s, np.array([0.0, 1, 1, 0]), np.array([0.0, 0, 1, 1])), 1)
    if not np.isfinite(q).all():
        return None
    return q, H, [c for c, k in zip(cells, keep) if k], float(np.sqrt((r ** 2).mean()))


def sums_of_homography(Ht, aw, ah, cell, n_per_cell, rng, box=(0.0, 0.0, 1.0, 1.0)):
    """Sum arrays in which every cell whose centre is the image of a unit-slide point inside `box` holds n_per_cell copies of ONE
    correspondence: the cell's centre (a multiple of 1/16) and its exact pre-image under the 3x3 Ht (unit slide -> pixels), rounded to
    2^-20.  The quad of such sums is Ht's up to that rounding."""
    gw, gh = E.grid(aw, ah, cell)
    sm = np.zeros((5, gh, gw), np.uint64)
    Hi = np.linalg.inv(Ht)
    for cy in range(gh):
        for cx in range(gw):
            X, Y = cx * cell + cell / 2.0, cy * cell + cell / 2.0
            if X >= aw or Y >= ah:
                continue
            p = Hi @ np.array([X, Y, 1.0])
            u, v = p[0] / p[2], p[1] / p[2]
            if not (box[0] <= u <= box[2] and box[1] <= v <= box[3]):
                continue
            k = int(n_per_cell if np.isscalar(n_per_cell) else rng.integers(n_per_cell[0], n_per_cell[1]))
            sm[:, cy, cx] = [k, k * int(round(X * 16)), k * int(round(Y * 16)), k * int(round(u * 1048576)), k * int(round(v * 1048576))]
    return sm


# ---- the constructed cases both test files use (tests/verify_cases.py builders) ----------------------------------------------------
REACHES = (8.0, 1.0)        # above and below small_cfg's ransac_threshold (3.0)


def near_case():
    """One page whose rows come in pairs of EQUAL descriptors 6 page pixels (4.8 frame pixels) apart in a direction of the pair's own, the pair's LOWER row being the
    farther one: every frame keypoint votes for both rows, RANSAC keeps the exact ones, both votes pass at reach 8, and the nearer — the
    higher row — gives the page point."""
    import verify_cases as VC
    c = VC.Case("NEAR", 76)
    pg = c.page(0, filler=0)
    decoys = c.points(pg, 40)
    ang = np.random.default_rng(760).uniform(0, 2 * np.pi, 40)             # (each pair its own direction: the decoys agree on no transform)
    true_xy = c.pages[pg].xy[decoys] + (6.0 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    rows = c.points(pg, 40, xy=true_xy, desc=c.pages[pg].desc[decoys])
    c.link(c.frame(0), pg, rows)
    return c


def tie_case():
    """One page whose rows come in pairs of equal descriptors at BIT-EQUAL points: both votes of a keypoint have the same d2 and the
    lower row gives the page point; the keypoint counts once."""
    import verify_cases as VC
    c = VC.Case("TIE", 77)
    pg = c.page(0, filler=0)
    rows = c.points(pg, 40)
    c.points(pg, 40, xy=c.pages[pg].xy[rows], desc=c.pages[pg].desc[rows])
    c.link(c.frame(0), pg, rows)
    return c


OUTSIDE_SIZE = (600, 338)


def outside_case():
    """One page declared 600x338 whose features include 12 points to the right of and below that size (a caller's features may hold
    any float): they are voted for, they pass, and they contribute nothing."""
    import verify_cases as VC
    c = VC.Case("OUTSIDE", 78)
    pg = c.page(0, filler=0)
    rng = np.random.default_rng(780)
    gx, gy = np.meshgrid(np.arange(45, OUTSIDE_SIZE[0] - 40, 41.0), np.arange(43, OUTSIDE_SIZE[1] - 40, 37.0))
    inside = (np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-3, 3, (gx.size, 2))).astype(np.float32)
    beyond = np.float32([[OUTSIDE_SIZE[0] - 0.5 + 11 * i, 60 + 20 * i] for i in range(6)] + [[80 + 60 * i, OUTSIDE_SIZE[1] - 0.5 + 9 * i] for i in range(6)])
    f = c.frame(0)
    c.link(f, pg, c.points(pg, len(inside), xy=inside))
    c.link(f, pg, c.points(pg, len(beyond), xy=beyond))
    c.page_sizes = {pg: OUTSIDE_SIZE}
    return c


def reach_case():
    """One page, 60 exact keypoints, 20 displaced by 2 px (inside ransac_threshold and reach 8; they pull the refined transform by
    at most 0.5 px, so they stay outside reach 1 and the exact ones inside) and 20 by 5 px (outside ransac_threshold, inside reach 8)."""
    import verify_cases as VC
    c = VC.Case("REACH", 79)
    pg = c.page(0, filler=0)
    f = c.frame(0)
    c.link(f, pg, c.points(pg, 60))
    c.link(f, pg, c.points(pg, 20), disp=(1.2, -1.6))
    c.link(f, pg, c.points(pg, 20), disp=(-3.0, 4.0), inlier=False)
    return c


def constructed_cases():
    """[(name, (case builder, arguments), page set or None, min_inliers)]: the evidence map's cases (verify_model 0 and 1, the ratio
    test, several votes of a keypoint of which one passes, frames without a contributor, a frame below min_inliers, a page set, frames
    of more keypoints than the window), then NEAR, TIE, pages of two sizes (tone_ref.sizes_case), OUTSIDE and REACH."""
    return E.constructed_cases() + [("NEAR", (near_case, ()), None, 0), ("TIE", (tie_case, ()), None, 0), ("SIZES", (T.sizes_case, ()), None, 0),
                                    ("OUTSIDE", (outside_case, ()), None, 0), ("REACH", (reach_case, ()), None, 0)]


def check_statements(name, reach, stats, got_sums, counted):
    """What each constructed case is there for, on the restatement's own figures."""
    n = int(got_sums[0].sum())
    if name == "T2-below":
        assert counted == 0 and n == 0, name
    elif name == "X1-none":
        pass                                       # (frames without a verdict: whether a slot has a model is the trace's to say)
    elif name == "NEAR" and reach > 3:
        assert stats["rivals"] == 40 and stats["nearer_is_higher_row"] == 40 and stats["ties"] == 0 and n == 40, stats
    elif name == "TIE":
        assert stats["ties"] == 40 and stats["passing"] == 80 and n == 40, stats
    elif name == "OUTSIDE":
        assert stats["outside"] == 12 and n > 40, stats
    elif name == "REACH":
        assert (n == 100) if reach > 5 else (60 <= n < 100), (reach, n)
    elif name == "SIZES":
        assert counted == 2 and n > 100
    else:
        assert counted >= 1 and n > 0, name


# ---- the keystone scene of "the use" (both test files) -------------------------------------------------------------------------------
# The evidence map's canvas texture (960x540) with its glyph pages (1600x900) shown over ONE fixed, visibly keystoned quad: where the
# page's corner pixel centres lie in the frame, top-left, top-right, bottom-right, bottom-left.  The left edge is 496 px long, the
# right one 442 px; the top edge falls by 26 px, the bottom one rises by 28.  Chosen on the CPU restatement: of four quads tried this
# is the one on which every frame has a contributor and the kept cells span three quarters of the slide both ways
# (test_placement_abi.py test_the_use_on_the_cpu asserts both); the glyph rows themselves cover v = 0.02 .. 0.91 of a page.
KEYSTONE_QUAD = ((40.0, 24.0), (920.0, 50.0), (908.0, 492.0), (52.0, 520.0))
# bound_px: twice the largest corner error the restatement gives on this scene (1.24 px), rounded up to a whole pixel
USE = dict(cell=32, min_inliers=12, reach=24.0, min_count=2, trim=3.0, rounds=4, n_pages=4, n_frames=8, nfeatures=3000, min_rating=12.0,
           bound_px=3.0)


def quad_homography(quad, w, h):
    """The 3x3 map from page pixel (x, y) of a w x h page to the frame, corners' pixel centres on the quad's corners."""
    src = [(0.0, 0.0), (w - 1.0, 0.0), (w - 1.0, h - 1.0), (0.0, h - 1.0)]
    A, b = [], []
    for (x, y), (X, Y) in zip(src, quad):
        A.append([x, y, 1, 0, 0, 0, -X * x, -X * y]); b.append(X)
        A.append([0, 0, 0, x, y, 1, -Y * x, -Y * y]); b.append(Y)
    return np.append(np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64)), 1.0).reshape(3, 3)


def keystone_scene(synth):
    """-> (pages uint8 [4, 900, 1600, 3], frames uint8 [8, 540, 960, 3], truth).  Frame i shows page i % 4 through the quad's
    homography, sampled bilinearly, over the static texture, with the frame's own faint noise (a camera's)."""
    pages, canvas, _ = E.canvas_scene(synth)
    tex = canvas[0].copy()
    tex[E.WIN_Y:E.WIN_Y + E.WIN_H, E.WIN_X:E.WIN_X + E.WIN_W] = tex[:E.WIN_H, :E.WIN_W][:, ::-1]      # (texture where the window was)
    ph, pw = pages.shape[1:3]
    Hi = np.linalg.inv(quad_homography(KEYSTONE_QUAD, pw, ph))
    X, Y = np.meshgrid(np.arange(E.CANVAS_W, dtype=np.float64), np.arange(E.CANVAS_H, dtype=np.float64))
    w = Hi[2, 0] * X + Hi[2, 1] * Y + Hi[2, 2]
    x = (Hi[0, 0] * X + Hi[0, 1] * Y + Hi[0, 2]) / w
    y = (Hi[1, 0] * X + Hi[1, 1] * Y + Hi[1, 2]) / w
    inside = (x >= 0) & (x <= pw - 1) & (y >= 0) & (y <= ph - 1)
    x0 = np.clip(np.floor(x), 0, pw - 2).astype(int); y0 = np.clip(np.floor(y), 0, ph - 2).astype(int)
    fx = np.clip(x - x0, 0, 1)[..., None]; fy = np.clip(y - y0, 0, 1)[..., None]
    rng = np.random.default_rng(2031)
    frames, truth = [], []
    for i in range(USE["n_frames"]):
        pg = pages[i % USE["n_pages"]].astype(np.float64)
        warped = (pg[y0, x0] * (1 - fx) + pg[y0, x0 + 1] * fx) * (1 - fy) + (pg[y0 + 1, x0] * (1 - fx) + pg[y0 + 1, x0 + 1] * fx) * fy
        f = np.where(inside[..., None], warped, tex.astype(np.float64)) + rng.normal(0, 1.5, tex.shape)
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        truth.append(i % USE["n_pages"])
    return pages, np.stack(frames), np.array(truth)


def corner_error(quad_):
    q = np.asarray(quad_, np.float64).reshape(4, 2)
    return float(np.sqrt(((q - np.array(KEYSTONE_QUAD)) ** 2).sum(1)).max())


def span_of(sm, kept, cell, min_count):
    """The share of the slide that the kept cells span along u and along v: the range of their unit-slide means plus one cell, the
    cell taken at the quad's mean edge length in that direction."""
    cells, u, v, _, _ = points(sm, min_count)
    k = [cells.index(c) for c in kept]
    q = np.array(KEYSTONE_QUAD)
    d = lambda a, b: float(np.hypot(*(q[a] - q[b])))
    ew, eh = (d(0, 1) + d(3, 2)) / 2, (d(0, 3) + d(1, 2)) / 2
    return float(u[k].max() - u[k].min()) + cell / ew, float(v[k].max() - v[k].min()) + cell / eh
