"""The numpy restatement of include/slideo_amd.h "Frame content box", written from that section: lit, the accumulator's lit counts
and frames, content, the row and column fills, n_content and the box.  The kernels (csrc/content.hip.h) are held to it, not it to
them."""
import numpy as np


def lit(image, level):
    """[h, w] bool: max(B, G, R) > level, in integers."""
    assert 0 <= int(level) <= 254
    return np.asarray(image, np.uint8).max(axis=2).astype(np.int32) > int(level)


class Accumulator:
    """The accumulator's state: `frames` and `lit` (uint32 [ah, aw]; None before the first frame)."""

    def __init__(self, level):
        assert 0 <= int(level) <= 254
        self.level, self.frames, self.lit = int(level), 0, None

    def observe(self, images):
        """images: [n, ah, aw, 3] uint8, the observed images of n frames."""
        for img in np.asarray(images, np.uint8):
            if self.lit is None:
                self.lit = np.zeros(img.shape[:2], np.uint32)
            assert img.shape[:2] == self.lit.shape
            self.lit += lit(img, self.level).astype(np.uint32)
            self.frames += 1
        return self


def counts(images, level):
    """-> (lit uint32 [ah, aw], frames) of ONE observation of all the images."""
    acc = Accumulator(level).observe(images)
    return acc.lit, acc.frames


def content(lit_counts, frames, min_share_ppm):
    """lit * 1000000 > min_share_ppm * frames in unsigned 64-bit integers: strict."""
    assert 0 <= int(min_share_ppm) <= 1000000
    return lit_counts.astype(np.uint64) * np.uint64(1000000) > np.uint64(int(min_share_ppm) * int(frames))


def fills(lit_counts, frames, min_share_ppm):
    """-> (row_fill uint32 [ah], col_fill uint32 [aw], n_content)"""
    c = content(lit_counts, frames, min_share_ppm)
    return c.sum(axis=1).astype(np.uint32), c.sum(axis=0).astype(np.uint32), int(c.sum())


def box(lit_counts, frames, min_share_ppm, min_fill_ppm):
    """-> ((x0, y0, x1, y1), n_content, row_fill, col_fill): the first content column, the last + 1, the same from the content rows;
    (0, 0, 0, 0) without a content row or without a content column."""
    assert frames > 0 and 0 <= int(min_fill_ppm) <= 1000000
    ah, aw = lit_counts.shape
    rf, cf, n = fills(lit_counts, frames, min_share_ppm)
    rows = np.nonzero(rf.astype(np.uint64) * np.uint64(1000000) > np.uint64(int(min_fill_ppm) * aw))[0]
    cols = np.nonzero(cf.astype(np.uint64) * np.uint64(1000000) > np.uint64(int(min_fill_ppm) * ah))[0]
    if len(rows) == 0 or len(cols) == 0:
        return (0, 0, 0, 0), n, rf, cf
    return (int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1), n, rf, cf


# ---- content the CPU and the GPU tests share ---------------------------------------------------------------------------------

LEVEL = 32


def level_frames(n, h, w, seed, level=LEVEL):
    """n frames of random content in the style of activity_ref.moving_frames (a random first frame, then about a third of the pixels
    step by up to +-14 per channel from one frame to the next) with the values pushed around `level`: about half of the pixels of
    every frame have each channel within +-3 of the level (maxima of exactly level and of level + 1 among them); from 5 rows and 7
    columns on, a band of rows at the top and of columns at the left stays at or below the level; and from 3 columns on two pixels
    are pinned to the level (not lit) and to level + 1 in one channel (lit) on every frame."""
    rng = np.random.default_rng(seed)
    f = np.empty((n, h, w, 3), np.uint8)
    f[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for i in range(1, n):
        step = rng.integers(-14, 15, (h, w, 3)) * (rng.random((h, w, 1)) < 0.33)
        f[i] = np.clip(f[i - 1].astype(np.int32) + step, 0, 255).astype(np.uint8)
    near = rng.random((n, h, w, 1)) < 0.5
    around = np.clip(level + rng.integers(-3, 4, (n, h, w, 3)), 0, 255).astype(np.uint8)
    f = np.where(near, around, f).astype(np.uint8)
    f[:, :h // 5] = np.minimum(f[:, :h // 5], level)
    f[:, :, :w // 7] = np.minimum(f[:, :, :w // 7], level)
    if w >= 3:
        f[:, h - 1, w - 1] = [level, level, level]
        f[:, h - 1, w - 2] = [0, level + 1, 0]
    return np.ascontiguousarray(f)


# ---- the matrix the CPU build of the kernels and the GPU run both cover --------------------------------------------------------

COUNT_SIZES = [(1, 1), (3, 2), (5, 7), (67, 9), (64, 8), (260, 17), (640, 360)]      # ragged rows, aw % 4 == 0, more than one block
BIG = (1920, 1080, 5)                                                              # one 1080p case, 5 frames
FRAME_COUNTS = (1, 2, 5, 9)                                                        # a single frame, the unroll's remainders
SPLIT = (1, 3, 5)                                                                  # the 9 frames over three calls / launches
READ_SIZES = [(1, 1), (5, 3), (67, 9), (640, 360), (4096, 3)]                      # the strip: the widest row, the longest column-fill array
READ_FRAMES = 4                                                                    # lit == 2 of 4 frames is exactly a share of 0.5
SHARES = (0.0, 0.5, 1.0)
FILLS = (0.0, 0.25, 1.0)


def strides(w):
    """row strides: tight; padded and no multiple of 4 (the byte path); padded, dword-aligned, with a ragged end"""
    odd = 3 * w + 5 if (3 * w + 5) % 4 else 3 * w + 6
    return {"tight": 3 * w, "odd": odd, "pad4": (3 * w + 3) // 4 * 4 + 4}


def layouts(n):
    """(stride kind, base offset in bytes) a size is run with at n frames: tight at +0 for every n; +1 byte, an odd stride and padded
    dword rows where the unroll runs (5, 9 frames)"""
    return [("tight", 0)] + ([("tight", 1), ("odd", 0), ("pad4", 0)] if n in (5, 9) else [])


def padded(frames, stride, ofs, fill=0x5A):
    """the frames in one uint8 buffer: `ofs` bytes, then n * h rows of `stride` bytes"""
    n, h, w, _ = frames.shape
    buf = np.full(ofs + n * h * stride, fill, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[ofs:], (n, h, w * 3), (h * stride, stride, 1))
    rows[:] = frames.reshape(n, h, w * 3)
    return buf


def read_frames(w, h):
    """READ_FRAMES frames for the read-out: level_frames, a frame-wide band lit in exactly 2 of the 4 frames (the equality of share
    0.5) and, from 5 columns on, a column lit in all of them (a fill of 1.0 is still not content: strict)."""
    f = level_frames(READ_FRAMES, h, w, w * 3 + h)
    if w >= 5:
        f[:, :, w - 2] = 255
    y = h // 2
    f[:2, y] = 200
    f[2:, y] = 0
    return f
