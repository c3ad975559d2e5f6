"""Numpy and Python-integer restatement of include/slideo_amd.h "Frame shading", written from the header: the gain field applied to a
BGR image and the field of per-cell sums (slideo_shading_field).  Everything is in integers; the tests compare by equality."""
import numpy as np

CELLS = (16, 32, 64)
# the sizes the tap and the host check run: one pixel, ragged rows of every remainder, a row of one thread, more than one cell either
# way at every cell size, an exact multiple of every cell, one column past it, several blocks
SIZES = [(1, 1), (3, 2), (4, 1), (17, 5), (64, 64), (65, 33), (640, 360)]


def strides(w):
    """Row strides in bytes: tight, one byte more (no row but the first is dword-aligned), five more."""
    return [3 * w, 3 * w + 1, 3 * w + 5]


def grid(aw, ah, cell):
    return -(-aw // cell), -(-ah // cell)


def identity(aw, ah, cell):
    gw, gh = grid(aw, ah, cell)
    return np.full((gh + 1, gw + 1), 256, np.uint16)


def random_field(aw, ah, cell, seed, lo=1, hi=65535):
    gw, gh = grid(aw, ah, cell)
    return np.random.default_rng(seed).integers(lo, hi + 1, (gh + 1, gw + 1), dtype=np.int64).astype(np.uint16)


def ramp_field(aw, ah, cell):
    """0.5 in the top-left corner to 3.0 in the bottom-right one."""
    gw, gh = grid(aw, ah, cell)
    j, i = np.mgrid[0:gh + 1, 0:gw + 1]
    return (128 + (640 * (i + j)) // max(1, gw + gh)).astype(np.uint16)


def gain_map(aw, ah, cell, gains):
    """int64 [ah, aw]: G of every pixel, the header's rule."""
    gw, gh = grid(aw, ah, cell)
    g = np.asarray(gains).astype(np.int64).reshape(gh + 1, gw + 1)
    assert g.min() >= 1 and g.max() <= 65535 and cell in CELLS
    sh = {16: 4, 32: 5, 64: 6}[cell]
    y, x = np.mgrid[0:ah, 0:aw]
    i, j = x // cell, y // cell
    fx, fy = x - i * cell, y - j * cell
    L = g[j, i] * (cell - fy) + g[j + 1, i] * fy
    R = g[j, i + 1] * (cell - fy) + g[j + 1, i + 1] * fy
    T = L * (cell - fx) + R * fx
    assert T.max() < 1 << 28
    return (T + cell * cell // 2) >> (2 * sh)


def apply(img, cell, gains):
    """out[c] = min(255, (in[c] * G + 128) >> 8) for uint8 [..., ah, aw, 3] images."""
    img = np.asarray(img, np.uint8)
    ah, aw = img.shape[-3], img.shape[-2]
    G = gain_map(aw, ah, cell, gains)
    v = img.astype(np.int64) * G[..., None]
    assert v.max() < 1 << 24
    return np.minimum(255, (v + 128) >> 8).astype(np.uint8)


def field(cnt, sum_f, sum_p, cell, min_count, min_gain, max_gain, smooth):
    """(gains uint16 [gh + 1, gw + 1], cells_used) by the five steps of the header in Python integers, or None where it refuses."""
    cnt = np.asarray(cnt)
    if cnt.ndim != 2:
        return None
    gh, gw = cnt.shape
    lim = -(-4096 // cell) if cell in CELLS else 0
    if cell not in CELLS or not (1 <= gw <= lim and 1 <= gh <= lim):
        return None
    if min_count < 1 or not 1 <= min_gain <= 256 <= max_gain <= 65535 or not 0 <= smooth <= 16:
        return None
    c = [[int(v) for v in r] for r in cnt]
    f = [[int(v) for v in r] for r in np.asarray(sum_f)]
    p = [[int(v) for v in r] for r in np.asarray(sum_p)]
    val = [[None] * gw for _ in range(gh)]
    used = 0
    for y in range(gh):
        for x in range(gw):
            if c[y][x] > 1 << 54 or f[y][x] > 765 * c[y][x] or p[y][x] > 765 * c[y][x]:
                return None
            if c[y][x] >= min_count and f[y][x] >= 1:
                r = (2 * 4096 * p[y][x] + f[y][x]) // (2 * f[y][x])
                val[y][x] = min(max(r, 16 * min_gain), 16 * max_gain)
                used += 1
    if used == 0:
        return None
    while any(v is None for row in val for v in row):
        nxt = [row[:] for row in val]
        for y in range(gh):
            for x in range(gw):
                if val[y][x] is not None:
                    continue
                nb = [val[b][a] for a, b in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)) if 0 <= a < gw and 0 <= b < gh and val[b][a] is not None]
                if nb:
                    nxt[y][x] = (2 * sum(nb) + len(nb)) // (2 * len(nb))
        val = nxt
    for _ in range(smooth):
        val = [[(2 * sum(val[min(max(y + dy, 0), gh - 1)][min(max(x + dx, 0), gw - 1)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 9) // 18
                for x in range(gw)] for y in range(gh)]
    out = np.empty((gh + 1, gw + 1), np.uint16)
    for j in range(gh + 1):
        for i in range(gw + 1):
            nb = [val[y][x] for y in (j - 1, j) for x in (i - 1, i) if 0 <= x < gw and 0 <= y < gh]
            node = (2 * sum(nb) + len(nb)) // (2 * len(nb))
            out[j, i] = min(max((node + 8) >> 4, min_gain), max_gain)
    return out, used


def falloff(frames, a=0.8):
    """The use case's recording: every frame multiplied by 1 - a * rho2, rho2 the mean of the squared normalised distances from the
    centre along x and y, rounded as clip(v * falloff + 0.5)."""
    frames = np.asarray(frames, np.uint8)
    H, W = frames.shape[-3], frames.shape[-2]
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rho2 = (((x - (W - 1) / 2) / (W / 2)) ** 2 + ((y - (H - 1) / 2) / (H / 2)) ** 2) / 2
    return np.clip(frames.astype(np.float64) * (1 - a * rho2)[..., None] + 0.5, 0, 255).astype(np.uint8)


# ---- the match shading map (include/slideo_amd.h "Match shading map") ----------------------------------------------------------------
MAX_FRAMES = 1 << 20
MAX_CELLS = 4096
# the scene of "the use" (evidence_ref.canvas_scene with the window under `falloff`) and its settings
USE = dict(cell=32, min_inliers=20, min_hits=20, flat=255, min_count=64, min_gain=64, max_gain=2048, smooth=1, a=0.8, min_rating=12.0)


def sums(frames, cell, *, min_inliers, min_hits, flat, model, thr, train_page, page_xy, pages, guard=True):
    """-> (sums uint64 [3, gh, gw]: cnt, sum_f, sum_p; frames_through, frames_counted) of tone_ref's frame records (all of one analysed
    size).  The sampler is tone_ref.frame_samples itself — which asserts the tone table's 1e-9 guards on its inputs — run on an image
    whose three bytes spell each pixel's index, so that every sample says where it fell."""
    import tone_ref as T
    assert cell in CELLS and min_inliers >= 0 and min_hits >= 1 and 0 <= flat <= 255 and len(frames) >= 1
    ah, aw = frames[0]["image"].shape[:2]
    gw, gh = grid(aw, ah, cell)
    assert gw * gh <= MAX_CELLS and aw * ah <= 1 << 24
    idx = np.arange(aw * ah, dtype=np.uint32).reshape(ah, aw)
    where = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], axis=2).astype(np.uint8)
    out = np.zeros((3, gh * gw), np.uint64)
    through = counted = 0
    for f in frames:
        assert f["image"].shape[:2] == (ah, aw)
        through += 1
        r = T.frame_samples(dict(f, image=where), min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=model, thr=thr,
                            train_page=train_page, page_xy=page_xy, pages=pages, guard=guard)
        if r is None:
            continue
        counted += 1
        at = r[0].astype(np.int64)
        at = at[:, 0] | (at[:, 1] << 8) | (at[:, 2] << 16)
        Yi, Xi = at // aw, at % aw
        k = (Yi // cell) * gw + Xi // cell
        fsum = np.asarray(f["image"], np.uint8)[Yi, Xi].astype(np.int64).sum(axis=1)
        psum = r[1].astype(np.int64).sum(axis=1)
        out[0] += np.bincount(k, minlength=gh * gw).astype(np.uint64)
        out[1] += np.bincount(k, weights=fsum.astype(np.float64), minlength=gh * gw).astype(np.uint64)      # (< 2^53: exact)
        out[2] += np.bincount(k, weights=psum.astype(np.float64), minlength=gh * gw).astype(np.uint64)
    assert through <= MAX_FRAMES
    return out.reshape(3, gh, gw), through, counted


def window_falloff(frames, a=USE["a"]):
    """The canvas scene's frames with the window alone under `falloff`, the surroundings left as they are."""
    import evidence_ref as E
    out = np.array(frames, np.uint8, copy=True)
    win = (slice(None), slice(E.WIN_Y, E.WIN_Y + E.WIN_H), slice(E.WIN_X, E.WIN_X + E.WIN_W))
    out[win] = falloff(out[win], a)
    return out
