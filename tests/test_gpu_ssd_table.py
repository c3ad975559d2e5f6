"""The SSD-table engine (csrc/ssd_table.hip.h) beyond its first wave tile: page_ssd_kernel through slideo_page_small_ssd and
slideo_page_small_ssd_valid with 130 pages of one size class — three 64-row page tiles, the last partial, and a second 128-row
block — against 1, 65 and 130 frames, and frame_gram_kernel through slideo_small_gram_ssd on the same images.

The reference is numpy in int64 (|a|^2 + |b|^2 - 2 a b^T over the valid bytes), every comparison is exact equality, and the taps'
own output is never the reference.

The deck (small_area 1200): page 0 a real 800x450 page, then 129 pages given as features (one keypoint each) with small images of
page 0's small size — page_small(0)'s, 46x25 here; 3 sw sh is no multiple of the K granule — and, at deck index 65, one 800x600
page of another size class, so a class position is not a deck index behind it and its column is UINT64_MAX.  The all-0 and the
all-255 image stand at class positions 1, 2, 128, 129 and at frames 1, 2, n - 2, n - 1: the largest SSD on both sides of every tile
boundary.  Class positions 1 .. 64 hold the first 64 of the 130 images S, so a column of the symmetric table is a column of the
rectangular one."""
import numpy as np
import pytest

import gate_mask_ref as gref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

AREA = 1200
NCLASS, OTHER = 130, 65                # pages of the class; the deck index of the page of another size
DECK_OF = [c if c < OTHER else c + 1 for c in range(NCLASS)]           # class position -> deck index
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
W, H = 640, 360


def _ssd(a, b, valid=None):
    """int64 [len(a), len(b)]: the SSD of every image of a with every image of b over the valid pixels (None: all)."""
    x = a.reshape(len(a), -1, 3).astype(np.int64)
    y = b.reshape(len(b), -1, 3).astype(np.int64)
    if valid is not None:
        x, y = x[:, valid.reshape(-1)], y[:, valid.reshape(-1)]
    x, y = x.reshape(len(x), -1), y.reshape(len(y), -1)
    return (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * (x @ y.T)


def _frames(S, n):
    """The first n images of S with the extremes at n - 2 and n - 1 too (S has them at 0, 1, 2)."""
    f = S[:n].copy()
    if n >= 4:
        f[n - 2], f[n - 1] = 0, 255
    return f


@pytest.fixture(scope="module")
def data(capi, synth):
    """-> (the real page, the 800x600 page, S [130, sh, sw, 3], the class's small images [130, sh, sw, 3])."""
    real = synth.pages(1, 800, 450)[0]
    tall = synth.pages(1, 800, 600, seed=77)[0]
    probe = capi.Matcher(small_cfg(capi, small_area=AREA))
    probe.add_pages([real])
    small0 = probe.page_small(0)
    probe.close()
    sh, sw = small0.shape[:2]
    assert sw * sh <= AREA and (sw * sh * 3) % 128 != 0, "no multiple of the K granule"
    rng = np.random.default_rng(19)
    S = rng.integers(0, 256, (NCLASS, sh, sw, 3), dtype=np.uint8)
    S[0], S[1], S[2], S[5] = 0, 255, 0, small0
    S[NCLASS - 2], S[NCLASS - 1] = 0, 255
    cls = rng.integers(0, 256, (NCLASS, sh, sw, 3), dtype=np.uint8)
    cls[0] = small0
    cls[1:65] = S[:64]
    cls[128], cls[129] = 0, 255
    assert not cls[1].any() and (cls[2] == 255).all()
    return real, tall, S, cls


def _deck(capi, data):
    real, tall, _, cls = data
    m = capi.Matcher(small_cfg(capi, small_area=AREA))
    m.add_pages([real])
    kp = np.zeros(1, capi.KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["response"] = 100.0, 100.0, 31.0, 1.0
    rng = np.random.default_rng(23)
    for c in range(1, NCLASS):
        if m.page_count == OTHER:
            m.add_pages([tall])
        m.add_page_features(800, 450, kp, rng.integers(0, 256, (1, 32), dtype=np.uint8), cls[c])
    m.finalize()
    assert m.page_count == NCLASS + 1
    assert all(np.array_equal(m.page_small(DECK_OF[c]), cls[c]) for c in (0, 1, 64, 65, 129)) and m.page_small(OTHER).shape != cls[0].shape
    return m


@pytest.fixture(scope="module")
def plain(capi, data):
    m = _deck(capi, data)
    yield m
    m.close()


@pytest.fixture(scope="module")
def masked(capi, oracle, data):
    """The same deck under a 640x360 mask with a rectangular hole, DETECT | GATE -> (matcher, validity map)."""
    mask = np.full((H, W), 255, np.uint8)
    mask[170:350, 380:630] = 0
    m = _deck(capi, data)
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(mask)
    valid, nv = gref.validity_map(oracle, mask, AREA)
    sh, sw = data[3].shape[1:3]
    assert valid.shape == (sh, sw) and 0 < nv < sw * sh
    got, got_n = m.frame_mask_small()
    assert np.array_equal(got, valid) and got_n == nv
    yield m, valid, nv
    m.close()


@pytest.fixture(scope="module")
def want_whole(data):
    """{n: int64 [n, 130]}: numpy's table of the n frames against the class."""
    return {n: _ssd(_frames(data[2], n), data[3]) for n in (1, 65, 130)}


def _check(got, want, n):
    assert got.shape == (n, NCLASS + 1) and got.dtype == np.uint64
    assert (got[:, OTHER] == U64_MAX).all(), "the page of another size"
    g = got[:, DECK_OF].astype(np.int64)
    bad = np.argwhere(g != want)
    assert len(bad) == 0, (len(bad), [(int(i), int(c), int(g[i, c]), int(want[i, c])) for i, c in bad[:6]])


@pytest.mark.parametrize("n", [1, 65, 130])
def test_page_small_ssd(plain, data, want_whole, n):
    """One tile; a second, partial frame tile; a second, partial frame block.  At this L and 130 x 130 K is split into chunks with
    a short last one: a wrong chunk edge is a wrong SSD here."""
    S, cls = data[2], data[3]
    want = want_whole[n]
    assert want.max() == 255 * 255 * 3 * cls.shape[1] * cls.shape[2], "the all-0 image against the all-255 image"
    own = [j for j in range(min(n, 64)) if n < 4 or j < n - 2]          # frame j is class page j + 1's small image
    assert own and all(want[j, j + 1] == 0 for j in own)
    if n > 5:
        assert want[5, 0] == 0, "the real page's own small image"
    _check(plain.page_small_ssd(_frames(S, n)), want, n)


def test_page_small_ssd_valid(masked, data, want_whole):
    m, valid, nv = masked
    S, cls = data[2], data[3]
    f = _frames(S, 65)
    want = _ssd(f, cls, valid)
    assert want.max() == 255 * 255 * 3 * nv and want[0, 1] == 0 and (want <= want_whole[65]).all() and (want < want_whole[65]).any()
    _check(m.page_small_ssd_valid(f), want, 65)
    _check(m.page_small_ssd(f), want_whole[65], 65)               # whole images on the same matcher: the map is not in the way


def test_small_gram_ssd_is_page_small_ssd(plain, data, want_whole):
    """frame_gram_kernel and page_ssd_kernel on the same images: class positions 1 .. 64 hold S[0:64]."""
    S = data[2]
    assert np.array_equal(_frames(S, NCLASS), S)
    gram = plain.small_gram_ssd(S)
    table = plain.page_small_ssd(S)
    assert gram.shape == (NCLASS, NCLASS) and gram.dtype == np.uint64
    assert np.array_equal(gram[:, :64], table[:, [DECK_OF[j + 1] for j in range(64)]])
    assert np.array_equal(gram.astype(np.int64), _ssd(S, S))
    _check(table, want_whole[NCLASS], NCLASS)
