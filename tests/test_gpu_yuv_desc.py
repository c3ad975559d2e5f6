"""YUV colour description (include/slideo_amd.h "YUV colour description") on the GPU: the conversion tap under every description
is bit-exact against the numpy restatement (tests/yuv_desc_ref.py) — all four (matrix, range) pairs, three depths, four formats,
tight, pitched and skewed layouts, so that the wide-load and the fallback paths of yuv420_to_bgr_desc_kernel both run —, and every
*_yuv420 call form under a description returns exactly what its *_bgr8 twin returns on the restatement's images."""
import numpy as np
import pytest

import yuv420_ref as ref8
import yuv_desc_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

DESCS = [(R.BT709, R.FULL, R.D10_MSB), (R.BT709, R.LIMITED, R.D8)]


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


# (the twelfth combination, all three fields 0, launches the 8-bit kernel: test_default_description_is_the_existing_path)
@pytest.mark.parametrize("desc", [(m, r, d) for d in R.DEPTHS for m, r in R.PAIRS if (m, r, d) != (0, 0, 0)], ids=lambda d: "m%d-r%d-d%d" % d)
def test_conversion_tap_bit_exact(capi, tap, desc):
    depth = desc[2]
    tap.set_yuv_description(*desc)
    assert tap.yuv_description() == desc
    k = 0
    for w, h in R.SIZES:
        for fmt in R.FORMATS:
            for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                k += 1
                buf = R.random_frame(w, h, L, fb, depth, 1000 * depth + k)
                got = tap.yuv420_to_bgr(buf, w, h, L)
                want = R.to_bgr(buf, w, h, L, desc)
                assert np.array_equal(got, want), (desc, fmt, w, h, name, np.argwhere(got != want)[:4])


def test_default_description_is_the_existing_path(capi, tap):
    """All three fields 0: the tap returns what the 8-bit path returns (this test's own run of it on a fresh matcher) and what the
    BT.601 restatement says."""
    fresh = capi.Matcher(small_cfg(capi))
    tap.set_yuv_description("bt709", "full", "10_lsb")
    tap.set_yuv_description("bt601", "limited", 8)
    assert tap.yuv_description() == (0, 0, 0)
    for w, h in R.SIZES:
        for fmt in R.FORMATS:
            for name, L, fb in R.layouts(capi, fmt, w, h, R.D8):
                buf = R.random_frame(w, h, L, fb, R.D8, w + h)
                got = tap.yuv420_to_bgr(buf, w, h, L)
                assert np.array_equal(got, fresh.yuv420_to_bgr(buf, w, h, L)), (fmt, w, h, name)
                assert np.array_equal(got, ref8.to_bgr(buf, w, h, L)) and np.array_equal(got, R.to_bgr(buf, w, h, L, (0, 0, 0)))
    fresh.close()


def test_layout_of_the_wrong_depth_is_refused(capi, tap):
    w, h = 64, 36
    L8, fb8 = capi.yuv420_layout("nv12", w, h)
    L16, fb16 = capi.yuv420_layout("nv12", w, h, bytes_per_sample=2)
    tap.set_yuv_description("bt709", "limited", "10_msb")
    c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(fb16, np.uint8), w, h, L8))
    assert c == 1 and "y_stride" in msg and "16-bit" in msg
    assert tap.yuv420_to_bgr(np.zeros(fb16, np.uint8), w, h, L16).shape == (h, w, 3)
    c, msg = _code(capi, lambda: tap.set_yuv_description(2, 0, 0))
    assert c == 1 and "matrix" in msg and tap.yuv_description() == (R.BT709, R.LIMITED, R.D10_MSB)      # the state before stays
    assert _code(capi, lambda: tap.set_yuv_description(0, 3, 0))[0] == 1
    assert _code(capi, lambda: tap.set_yuv_description(0, 0, 5))[0] == 1
    tap.set_yuv_description()


def _layout_for(capi, desc, w, h, fmt="nv12"):
    b = R.bps(desc[2])
    return capi.yuv420_layout(fmt, w, h, pitch=-(-w * b // 256) * 256, row_align=16, bytes_per_sample=b)


@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.repeat(frames, 2, axis=0)                            # every frame twice: changed and unchanged flags both occur
    return pages, seq


@pytest.fixture(scope="module", params=DESCS, ids=["bt709-full-p010", "bt709-limited-8"])
def described(request, capi, deck):
    """One matcher under the description, the sequence as 4:2:0 frames under it, and the restatement's BGR images."""
    desc = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    L, fb = _layout_for(capi, desc, w, h)
    yuv = R.frames_to_yuv(seq, L, fb, desc)
    bgr = np.stack([R.to_bgr(f, w, h, L, desc) for f in yuv])
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    m.set_yuv_description(*desc)
    yield desc, m, yuv, L, bgr, w, h
    m.close()


def test_the_restatements_images_are_close_to_the_source(described, deck):
    """(The forward transform of the test is sane: the images under the right description are the source frames within rounding.)"""
    _, _, _, _, bgr, _, _ = described
    err = np.abs(bgr.astype(np.int32) - deck[1].astype(np.int32))
    assert np.median(err) <= 2


def test_match_frames_host_device_and_streaming(capi, described):
    import torch
    desc, m, yuv, L, bgr, w, h = described
    n, fs = yuv.shape
    want = m.match_frames(bgr)
    c_want = [m.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).mean() >= 0.5
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    d = torch.from_numpy(yuv).cuda()
    assert _same(m.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, fs), want)
    got, pend = [], []
    for i in range(0, n, 4):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_yuv420_dev(d.data_ptr() + i * fs, min(4, n - i), w, h, L, fs))
    # a busy matcher refuses the setter, and the description in force stays
    c, _ = _code(capi, lambda: m.set_yuv_description())
    assert c == 4 and m.yuv_description() == desc
    got += [m.collect(t) for t in pend]
    assert _same(np.concatenate(got), want)


def test_changed_mask_and_gated_calls(capi, described):
    desc, m, yuv, L, bgr, w, h = described
    ch, sim, last = m.changed_mask(bgr)
    assert ch.any() and not ch.all()
    yc, ys, yl = m.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
    yc2, ys2, yl2 = m.changed_mask_yuv420(yuv[3:], w, h, L, prev_small=yl)
    ch2, sim2, last2 = m.changed_mask(bgr[3:], prev_small=last)
    assert np.array_equal(yc2, ch2) and _same(ys2, sim2) and np.array_equal(yl2, last2)
    # the gate: two calls continuing one state, and a state primed from one frame
    m.gate_reset()
    want = [m.match_changed_frames(bgr[:5]), m.match_changed_frames(bgr[5:])]
    want_small = m.gate_last_small()
    m.gate_reset()
    got = [m.match_changed_frames_yuv420(yuv[:5], w, h, L), m.match_changed_frames_yuv420(yuv[5:], w, h, L)]
    for g, wnt in zip(got, want):
        assert np.array_equal(g[0], wnt[0]) and _same(g[1], wnt[1]) and _same(g[2], wnt[2])
    assert np.array_equal(m.gate_last_small(), want_small)
    m.gate_reset_from_frame(bgr[2])
    a = m.match_changed_frames(bgr[3:6])
    primed = m.gate_last_small()
    m.gate_reset_from_frame_yuv420(yuv[2], w, h, L)
    b = m.match_changed_frames_yuv420(yuv[3:6], w, h, L)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]) and np.array_equal(m.gate_last_small(), primed)
    m.gate_reset()


def test_group_of_two_members(capi, described, deck):
    desc, m, yuv, L, bgr, w, h = described
    want = m.match_frames(bgr)
    ch, sim, last = m.changed_mask(bgr)
    m.gate_reset()
    gated = m.match_changed_frames(bgr)
    m.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    g.set_yuv_description(*desc)
    assert g.yuv_description() == desc
    assert _same(g.match_frames_yuv420(yuv, w, h, L), want)
    gc, gs, gl = g.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    got = g.match_changed_frames_yuv420(yuv, w, h, L)
    assert np.array_equal(got[0], gated[0]) and _same(got[1], gated[1]) and _same(got[2], gated[2])
    # the group's setter validates before it changes any member
    c, _ = _code(capi, lambda: g.set_yuv_description(0, 0, 7))
    assert c == 1 and g.yuv_description() == desc
    g.close()


def test_under_a_working_size_and_under_a_region(capi, described):
    desc, m, yuv, L, bgr, w, h = described
    m.set_working_size(480, 270)
    try:
        want = m.match_frames(bgr[::2])
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), want)
        ch, sim, last = m.changed_mask(bgr[:6])
        yc, ys, yl = m.changed_mask_yuv420(yuv[:6], w, h, L)
        assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last) and last.shape[0] * last.shape[1] <= 120000
    finally:
        m.set_working_size(0, 0)
    m.set_frame_region(w, h, [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)], 480, 270)
    try:
        want = m.match_frames(bgr[::2])
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), want)
        m.gate_reset()
        a = m.match_changed_frames(bgr[:6])
        m.gate_reset()
        b = m.match_changed_frames_yuv420(yuv[:6], w, h, L)
        assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])
    finally:
        m.clear_frame_region()
        m.gate_reset()


def test_back_to_the_default_equals_a_fresh_matcher(capi, deck):
    pages, seq = deck
    n, h, w, _ = seq.shape
    L, fb = capi.yuv420_layout("nv12", w, h, pitch=768, row_align=16)
    yuv = ref8.frames_to_yuv(seq[:8], L, fb)

    def results(m):
        v = m.match_frames_yuv420(yuv, w, h, L)
        return v, m.changed_mask_yuv420(yuv, w, h, L), m.yuv420_to_bgr(yuv[0], w, h, L)
    ms = []
    for _ in range(2):
        m = capi.Matcher(small_cfg(capi))
        m.add_pages(list(pages))
        m.finalize()
        ms.append(m)
    ms[1].set_yuv_description("bt709", "full", "10_msb")
    ms[1].set_yuv_description("bt601", "limited", 8)
    a, b = results(ms[0]), results(ms[1])
    assert _same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[2], ref8.to_bgr(yuv[0], w, h, L))
    for m in ms:
        m.close()


def test_setting_it_ends_the_kept_frames_and_resets_the_gate(capi, described):
    desc, m, yuv, L, bgr, w, h = described
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames_yuv420(yuv[:2], w, h, L)
    assert m.gate_last_small().ndim == 3
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    m.set_yuv_description(*desc)                                  # (the same values: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames_yuv420(yuv[1:3], w, h, L)
    assert ch[0]                                                  # the first gated frame after it is changed
    m.gate_reset()
