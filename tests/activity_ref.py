"""The numpy restatement of include/slideo_amd.h "Frame activity map", written from that section: moved, count, pairs, active,
mask, n_active and n_masked.  The kernels (csrc/activity.hip.h) are held to it, not it to them."""
import numpy as np


def moved(a, b, delta):
    """[h, w] bool: |a.B-b.B| + |a.G-b.G| + |a.R-b.R| > delta, in integers."""
    sad = np.abs(a.astype(np.int32) - b.astype(np.int32)).sum(axis=2)
    return sad > int(delta)


class Accumulator:
    """The accumulator's state: `last` (None before the first frame), `pairs` and `count` (uint32 [ah, aw])."""

    def __init__(self, delta):
        assert 0 <= int(delta) <= 765
        self.delta, self.last, self.pairs, self.count = int(delta), None, 0, None

    def observe(self, images):
        """images: [n, ah, aw, 3] uint8, the observed images of n frames, in submission order."""
        for img in np.asarray(images, np.uint8):
            if self.last is None:
                self.count = np.zeros(img.shape[:2], np.uint32)
            else:
                assert img.shape == self.last.shape
                self.count += moved(self.last, img, self.delta).astype(np.uint32)
                self.pairs += 1
            self.last = img.copy()
        return self


def counts(images, delta):
    """-> (count uint32 [ah, aw], pairs) of ONE observation of all the images."""
    acc = Accumulator(delta).observe(images)
    return acc.count, acc.pairs


def active(count, pairs, max_share_ppm):
    """count * 1000000 > max_share_ppm * pairs in unsigned 64-bit integers: strict."""
    return count.astype(np.uint64) * np.uint64(1000000) > np.uint64(int(max_share_ppm) * int(pairs))


def mask(count, pairs, max_share_ppm, grow):
    """-> (mask uint8 [ah, aw]: 0 iff an active pixel lies within `grow` in x AND in y, else 255; n_active; n_masked)"""
    assert pairs > 0 and 0 <= max_share_ppm <= 1000000 and 0 <= grow <= 64
    act = active(count, pairs, max_share_ppm)
    h, w = act.shape
    # the square of every DISTINCT active row / column pair would be slow; dilate per axis with clipped windows instead, which is the
    # same set: |x'-x| <= grow and |y'-y| <= grow are independent conditions on one active pixel (x', y')
    cx = np.zeros((h, w + 1), np.int64)
    cx[:, 1:] = np.cumsum(act, axis=1)
    lo = np.clip(np.arange(w) - grow, 0, w - 1)
    hi = np.clip(np.arange(w) + grow, 0, w - 1)
    in_x = (cx[:, hi + 1] - cx[:, lo]) > 0                        # some active pixel of the row within grow columns
    cy = np.zeros((h + 1, w), np.int64)
    cy[1:] = np.cumsum(in_x, axis=0)
    lo = np.clip(np.arange(h) - grow, 0, h - 1)
    hi = np.clip(np.arange(h) + grow, 0, h - 1)
    hit = (cy[hi + 1] - cy[lo]) > 0
    out = np.where(hit, 0, 255).astype(np.uint8)
    return out, int(act.sum()), int(hit.sum())


def mask_by_definition(count, pairs, max_share_ppm, grow):
    """The definition word for word (one square per active pixel): for small images, to check `mask` itself."""
    act = active(count, pairs, max_share_ppm)
    h, w = act.shape
    out = np.full((h, w), 255, np.uint8)
    for y, x in zip(*np.nonzero(act)):
        out[max(y - grow, 0):y + grow + 1, max(x - grow, 0):x + grow + 1] = 0
    return out, int(act.sum()), int((out == 0).sum())


# ---- content the CPU and the GPU tests share ---------------------------------------------------------------------------------

def moving_frames(n, h, w, seed):
    """n frames in which about a third of the pixels change from one frame to the next, by sums on both sides of delta 24 (and
    exactly 24 and 25 somewhere), and a block that changes on every frame."""
    rng = np.random.default_rng(seed)
    f = np.empty((n, h, w, 3), np.uint8)
    f[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for i in range(1, n):
        step = rng.integers(-14, 15, (h, w, 3)) * (rng.random((h, w, 1)) < 0.33)
        f[i] = np.clip(f[i - 1].astype(np.int32) + step, 0, 255).astype(np.uint8)
        f[i, h // 2:h // 2 + 9, w - 7:] = rng.integers(0, 256, (min(9, h - h // 2), 7, 3), dtype=np.uint8)
        for (y, x), d in (((0, 0), [8, 8, 8]), ((h - 1, w - 1), [9, 8, 8])):        # SADs of exactly 24 and 25
            p = f[i - 1, y, x].astype(np.int32)
            f[i, y, x] = p + d if p.max() < 200 else p - d
    return f
