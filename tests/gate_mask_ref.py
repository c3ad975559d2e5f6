"""The frame mask's GATE scope (include/slideo_amd.h "Frame mask scope") restated in numpy: the validity map from the CPU
to_small_image, the masked SSD from small images, the similarity in the float types of changed_similarity() (csrc/runtime.hpp) and
the threshold by the same bisection.  Nothing here calls the library under test."""
import numpy as np

INT64_MAX = (1 << 63) - 1


def validity_map(oracle, mask, small_area=120000):
    """-> (valid bool [sh, sw], n_valid): B = the mask binarised and replicated to three channels, S = to_small_image(B); a small
    pixel is valid iff S[y, x, 0] == 255."""
    mask = np.asarray(mask)
    b = np.where(mask != 0, 255, 0).astype(np.uint8)
    s = oracle.small_image(np.ascontiguousarray(np.repeat(b[:, :, None], 3, axis=2)), small_area)
    valid = s[:, :, 0] == 255
    return valid, int(valid.sum())


def small_images(oracle, frames, small_area=120000):
    return np.stack([oracle.small_image(f, small_area) for f in frames])


def masked_ssd(a, b, valid):
    """The sum over the valid pixels' three channels of (a - b)^2, an exact integer."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum(axis=2)[valid].sum())


def similarity(ssd, n):
    """changed_similarity() with n pixels: a float64 sqrt of the SSD, a float32 sqrt((255 * 255 * 3) * (float)n), then
    1 - (float)e / max_error in float32."""
    e = np.sqrt(np.float64(ssd))
    max_error = np.sqrt(np.float32(np.float32(255.0) * np.float32(255.0) * np.float32(3.0)) * np.float32(n))
    assert max_error.dtype == np.float32
    out = np.float32(1.0) - np.float32(e) / max_error
    assert out.dtype == np.float32
    return out


def is_changed(ssd, n, changed_similarity):
    return bool(similarity(ssd, n) < np.float32(changed_similarity))


def threshold(changed_similarity, n):
    """The smallest SSD that counts as changed over n pixels: the library's bisection over the expression above.  INT64_MAX when
    even the maximal SSD is unchanged, 0 when SSD 0 already is changed."""
    max_ssd = 255 * 255 * 3 * int(n)
    if not is_changed(max_ssd, n, changed_similarity):
        return INT64_MAX
    if is_changed(0, n, changed_similarity):
        return 0
    lo, hi = 0, max_ssd
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if is_changed(mid, n, changed_similarity):
            hi = mid
        else:
            lo = mid
    return hi


def flags(smalls, valid, changed_similarity, prev_small=None):
    """MarkSimilarIter over small images under the validity map -> (changed bool [n], similarity f32 [n]).  Without prev_small the
    first frame compares as 0.0 and is changed.  valid None: the whole image (the unmasked gate)."""
    if valid is None:
        valid = np.ones(smalls.shape[1:3], bool)
    n = int(valid.sum())
    ch = np.zeros(len(smalls), bool)
    sim = np.zeros(len(smalls), np.float32)
    prev = prev_small
    for i, s in enumerate(smalls):
        sim[i] = np.float32(0.0) if prev is None else similarity(masked_ssd(prev, s, valid), n)
        ch[i] = sim[i] < np.float32(changed_similarity)
        prev = s
    return ch, sim
