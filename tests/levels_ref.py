"""Numpy restatement of include/slideo_amd.h "Frame levels", written from the header: the table applied to a BGR image, the
per-channel histogram of the observed images, the points of a histogram and the stretch table of two points.  Everything is in
integers; the tests compare by equality."""
import numpy as np

MAX_PPM = 1000000

# the sizes the tap and the host check run: one pixel, ragged rows of every remainder, a full thread row, more than one block
# along a row (64 threads x 4 pixels = 256 columns do not occur below 640), several row tiles
SIZES = [(1, 1), (3, 2), (4, 1), (61, 47), (64, 48), (130, 33), (640, 360)]


def strides(w):
    """Row strides in bytes: tight, one byte more (no row but the first is dword-aligned), five more."""
    return [3 * w, 3 * w + 1, 3 * w + 5]


def identity():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def apply(img, lut):
    """out[..., c] = lut[c][img[..., c]] for uint8 [..., 3] images (B, G, R last)."""
    img = np.asarray(img, np.uint8)
    lut = np.asarray(lut, np.uint8).reshape(3, 256)
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = lut[c][img[..., c]]
    return out


def histogram(imgs):
    """uint64 [3, 256]: the samples of every value per channel of uint8 [..., 3] images."""
    imgs = np.asarray(imgs, np.uint8).reshape(-1, 3)
    return np.stack([np.bincount(imgs[:, c], minlength=256).astype(np.uint64) for c in range(3)])


def value_at(hist256, rank):
    """The value of the sample of ascending rank `rank` (0-based) of one channel's histogram."""
    below = 0
    for v in range(256):
        below += int(hist256[v])
        if rank < below:
            return v
    raise ValueError("rank %d of %d samples" % (rank, below))


def points(hist, low_ppm, high_ppm):
    """(lo [3], hi [3]): per channel the value of the sample of rank floor(total * low_ppm / 1e6) and of rank total - 1 -
    floor(total * high_ppm / 1e6), either rank clamped into 0 .. total - 1; Python integers, no rounding anywhere."""
    lo, hi = [], []
    for c in range(3):
        h = [int(v) for v in np.asarray(hist).reshape(3, 256)[c]]
        total = sum(h)
        assert total > 0
        rl = min(total * int(low_ppm) // MAX_PPM, total - 1)
        cut = min(total * int(high_ppm) // MAX_PPM, total - 1)
        lo.append(value_at(h, rl))
        hi.append(value_at(h, total - 1 - cut))
    return lo, hi


def stretch_lut(lo, hi):
    """uint8 [3, 256]: lut[c][x] = clamp(floor((510 (x - lo) + (hi - lo)) / (2 (hi - lo))), 0, 255); needs 0 <= lo < hi <= 255."""
    out = np.empty((3, 256), np.uint8)
    for c in range(3):
        l, h = int(lo[c]), int(hi[c])
        assert 0 <= l < h <= 255
        d = h - l
        for x in range(256):
            out[c, x] = min(255, max(0, (510 * (x - l) + d) // (2 * d)))      # (Python's // floors)
    return out


def stretch_row(l, h):
    """One channel of stretch_lut, vectorised (for the sweep over all pairs)."""
    x = np.arange(256, dtype=np.int64)
    d = h - l
    return np.clip(np.floor_divide(510 * (x - l) + d, 2 * d), 0, 255).astype(np.uint8)


def random_lut(seed):
    """A random table per channel (not monotonic, not a permutation: any table is a table)."""
    return np.random.default_rng(seed).integers(0, 256, (3, 256), dtype=np.uint8)


def darken(frames, gain=0.3, offset=30.0):
    """The dim recording of the use case."""
    return np.clip(np.asarray(frames).astype(np.float32) * gain + offset, 0, 255).astype(np.uint8)
