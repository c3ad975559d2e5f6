"""frame_gram_kernel and the operand kernels on their own: slideo_small_gram_ssd (include/slideo_amd.h "Gate reference") against numpy's
all-pairs SSD (tests/gate_anchor_ref.py all_pairs_ssd, exact), every comparison exact equality.

Shapes: n = 1 (no pair), 2, 65 (a second, partial 64-row wave tile: one tile off the diagonal) and 130 (a second, partial 128-row
block: blocks on and off the diagonal and one wholly below it); L = 3 sw sh = 105 (below one 128-byte K granule), 2139 (several
1 KiB minimum chunks and a ragged, dword-unaligned tail: 2139 = 16 * 133 + 11) and 358 197 (the small image of a 640x360 frame: K
split over several chunks).  Contents: random bytes, and all-0 and all-255 images twice each — the largest SSD, and against
themselves a product of 16 384 per byte, an i32 accumulator's designed limit of 2^30 per K chunk — at indices on both sides of the
tile boundary.
use_valid: a validity map exists only for frames of at least small_area pixels, so its small size is about small_area — here
461x259; the other two sizes are the tap's SLIDEO_ERR_INVALID_ARG, and no map at all is SLIDEO_ERR_STATE."""
import numpy as np
import pytest

import gate_anchor_ref as aref
import gate_mask_ref as gref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

SIZES = [(7, 5), (31, 23), (461, 259)]
NS = [1, 2, 65, 130]
W, H = 640, 360


def _images(n, sw, sh):
    rng = np.random.default_rng(1000 * sw + n)
    s = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    if n == 1:
        s[0] = 0
    elif n == 2:
        s[0], s[1] = 0, 255
    else:
        for i, v in ((1, 0), (2, 255), (n - 2, 0), (n - 1, 255)):     # (n - 2, n - 1: in the last, partial tile)
            s[i] = v
    return s


@pytest.fixture(scope="module")
def plain(capi):
    m = capi.Matcher(small_cfg(capi))                            # the tap needs no pages
    yield m
    m.close()


@pytest.fixture(scope="module")
def masked(capi, oracle):
    mask = np.full((H, W), 255, np.uint8)
    mask[190:350, 390:630] = 0
    m = capi.Matcher(small_cfg(capi))
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(mask)
    valid, nv = gref.validity_map(oracle, mask)
    assert valid.shape == (259, 461) and 0 < nv < valid.size
    got, got_n = m.frame_mask_small()
    assert np.array_equal(got, valid) and got_n == nv
    yield m, valid
    m.close()


def _check(got, want, n):
    assert got.shape == (n, n) and got.dtype == np.uint64
    g = got.astype(np.int64)
    assert np.array_equal(g, g.T), "symmetric"
    assert not np.diagonal(g).any(), "zero diagonal"
    bad = np.argwhere(g != want)
    assert len(bad) == 0, (len(bad), [(int(i), int(j), int(g[i, j]), int(want[i, j])) for i, j in bad[:6]])


@pytest.mark.parametrize("sw,sh", SIZES)
@pytest.mark.parametrize("n", NS)
def test_whole_images(plain, n, sw, sh):
    s = _images(n, sw, sh)
    want = aref.all_pairs_ssd(s)
    if n >= 2:
        assert want.max() == 255 * 255 * 3 * sw * sh, "the all-0 and the all-255 image: the largest SSD"
    _check(plain.small_gram_ssd(s), want, n)


@pytest.mark.parametrize("n", NS)
def test_valid_pixels(masked, n):
    m, valid = masked
    s = _images(n, 461, 259)
    want = aref.all_pairs_ssd(s, valid)
    if n >= 2:
        assert want.max() == 255 * 255 * 3 * int(valid.sum())
    _check(m.small_gram_ssd(s, use_valid=True), want, n)
    if n == 65:                                                  # the same matcher, whole images: the map is not in the way
        _check(m.small_gram_ssd(s), aref.all_pairs_ssd(s), n)


def test_refusals(capi, plain, masked):
    m, _ = masked
    for sw, sh in SIZES[:2]:
        with pytest.raises(capi.SlideoError) as e:
            m.small_gram_ssd(_images(2, sw, sh), use_valid=True)
        assert e.value.code == 1, "another size than the map's"
    with pytest.raises(capi.SlideoError) as e:
        plain.small_gram_ssd(_images(2, 461, 259), use_valid=True)
    assert e.value.code == 4, "no validity map in force"
    with pytest.raises(capi.SlideoError) as e:
        plain.small_gram_ssd(np.zeros((2, 400, 400, 3), np.uint8))
    assert e.value.code == 1, "beyond small_area"
    assert plain.small_gram_ssd(np.zeros((0, 5, 7, 3), np.uint8)).shape == (0, 0)
