"""YUV sampling (include/slideo_amd.h "YUV sampling") on the GPU: the conversion tap under 4:2:2, 4:4:4 and packed 4:2:2 is
bit-exact against the numpy restatement (tests/yuv_sampling_ref.py) — every format of each sampling, its depths, tight, pitched and
skewed layouts, so that every wide load of yuv_sampled_to_bgr_kernel and its fallback run —, the default sampling is the existing
path, and every call form under a sampling returns exactly what its *_bgr8 twin returns on the restatement's images."""
import ctypes as C

import numpy as np
import pytest

import yuv420_ref as ref8
import yuv_desc_ref as D
import yuv_sampling_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

PAIRS = [(D.BT601, D.LIMITED), (D.BT709, D.FULL)]
# (sampling name, sampling, format, description)
FORMS = [("444", R.S444, "i444", (D.BT601, D.LIMITED, D.D8)), ("422", R.S422, "nv16", (D.BT709, D.LIMITED, D.D10_MSB)),
         ("422_packed", R.S422P, "uyvy", (D.BT601, D.LIMITED, D.D8))]


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


@pytest.mark.parametrize("sampling,depth", [(s, d) for s in R.SAMPLINGS for d in R.DEPTHS[s]], ids=lambda v: str(v))
def test_conversion_tap_bit_exact(capi, tap, sampling, depth):
    tap.set_yuv_description()
    tap.set_yuv_sampling(R.SAMPLING_NAMES[sampling])
    assert tap.yuv_sampling() == sampling
    k = 0
    for matrix, rng in PAIRS:
        desc = (matrix, rng, depth)
        tap.set_yuv_description(*desc)
        assert tap.yuv_description() == desc and tap.yuv_sampling() == sampling
        for w, h in R.sizes(sampling):
            for fmt in R.FORMATS[sampling]:
                for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                    k += 1
                    buf = R.random_frame(w, h, L, fb, depth, sampling, 1000 * depth + k)
                    got = tap.yuv420_to_bgr(buf, w, h, L)
                    want = R.to_bgr(buf, w, h, L, desc, sampling)
                    assert np.array_equal(got, want), (desc, fmt, w, h, name, np.argwhere(got != want)[:4])
    if sampling != R.S444:                          # odd widths are refused (and a 4:4:4 frame of 7 x 5 ran above)
        L, fb = R.make_layout(capi, R.FORMATS[sampling][0], 8, 3, D.bps(depth))
        c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(fb, np.uint8), 7, 3, L))
        assert c == 5 and "even" in msg
    tap.set_yuv_description()
    tap.set_yuv_sampling("420")


def test_default_sampling_is_the_existing_path(capi, tap):
    """After 444 and back: the tap over yuv_desc_ref's matrix returns what a fresh matcher returns and what the 4:2:0 restatement
    says; yuv_description() is a 3-tuple the sampling setter does not touch."""
    fresh = capi.Matcher(small_cfg(capi))
    tap.set_yuv_description("bt709", "full", "10_msb")
    tap.set_yuv_sampling("444")
    assert tap.yuv_description() == (D.BT709, D.FULL, D.D10_MSB) and tap.yuv_sampling() == 2
    tap.set_yuv_sampling("420")
    assert tap.yuv_description() == (D.BT709, D.FULL, D.D10_MSB) and tap.yuv_sampling() == 0
    tap.set_yuv_description()
    assert tap.yuv_description() == (0, 0, 0) and fresh.yuv_sampling() == 0
    for w, h in D.SIZES:
        for fmt in D.FORMATS:
            for name, L, fb in D.layouts(capi, fmt, w, h, D.D8):
                buf = D.random_frame(w, h, L, fb, D.D8, w + h)
                got = tap.yuv420_to_bgr(buf, w, h, L)
                assert np.array_equal(got, fresh.yuv420_to_bgr(buf, w, h, L)), (fmt, w, h, name)
                assert np.array_equal(got, ref8.to_bgr(buf, w, h, L)) and np.array_equal(got, D.to_bgr(buf, w, h, L, (0, 0, 0)))
    # and under a description: the 4:2:0 description kernel, as before
    desc = (D.BT709, D.LIMITED, D.D10_LSB)
    tap.set_yuv_description(*desc)
    fresh.set_yuv_description(*desc)
    for fmt in D.FORMATS:
        for name, L, fb in D.layouts(capi, fmt, 66, 34, D.D10_LSB):
            buf = D.random_frame(66, 34, L, fb, D.D10_LSB, 7)
            got = tap.yuv420_to_bgr(buf, 66, 34, L)
            assert np.array_equal(got, fresh.yuv420_to_bgr(buf, 66, 34, L)) and np.array_equal(got, D.to_bgr(buf, 66, 34, L, desc))
    tap.set_yuv_description()
    fresh.close()


def test_refusals(capi, tap):
    w, h = 64, 36
    tap.set_yuv_sampling("444")
    L, fb = capi.yuv420_layout("i420", w, h, pitch=2 * w)          # a 4:2:0 layout: the U plane, of h rows now, runs into V
    c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(4 * w * h, np.uint8), w, h, L))
    assert c == 1 and "overlaps" in msg and "yuv444" in msg
    tap.set_yuv_sampling("422")
    P, pb = capi.yuv_layout("yuy2", w, h)
    c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(pb, np.uint8), w, h, P))
    assert c == 1 and "uv_step 4" in msg and "yuv422" in msg
    c, msg = _code(capi, lambda: tap.set_yuv_sampling(4))
    assert c == 1 and "yuv sampling" in msg and tap.yuv_sampling() == 1                   # the state before stays
    assert _code(capi, lambda: tap.set_yuv_sampling("411"))[0] == 1
    tap.set_yuv_sampling("420")
    c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(pb, np.uint8), w, h, P))
    assert c == 1 and "uv_step 4" in msg and "yuv420" in msg
    # packed is 8-bit: whichever call would complete the pair is refused, and the values before stay
    tap.set_yuv_sampling("422_packed")
    c, msg = _code(capi, lambda: tap.set_yuv_description("bt709", "limited", "10_msb"))
    assert c == 5 and tap.yuv_description() == (0, 0, 0) and tap.yuv_sampling() == 3
    tap.set_yuv_sampling("420")
    tap.set_yuv_description("bt709", "limited", "10_msb")
    c, msg = _code(capi, lambda: tap.set_yuv_sampling("422_packed"))
    assert c == 5 and tap.yuv_sampling() == 0 and tap.yuv_description() == (D.BT709, D.LIMITED, D.D10_MSB)
    tap.set_yuv_description()
    # the group's setter validates every member before it changes any
    g = capi.Group(small_cfg(capi), [0, 0])
    g.set_yuv_sampling("422")
    assert g.yuv_sampling() == 1
    c, _ = _code(capi, lambda: g.set_yuv_sampling(9))
    assert c == 1 and g.yuv_sampling() == 1
    member1 = capi.lib().slideo_group_member(g._h, 1)
    assert capi.lib().slideo_matcher_set_yuv_description(member1, 1, 0, 1) == 0            # one member at 10 bits: it refuses packed
    c, _ = _code(capi, lambda: g.set_yuv_sampling("422_packed"))
    assert c == 5 and g.yuv_sampling() == 1
    v = C.c_int32()
    assert capi.lib().slideo_matcher_yuv_sampling(member1, C.byref(v)) == 0 and v.value == 1          # no member changed
    g.close()


@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.repeat(frames, 2, axis=0)                            # every frame twice: changed and unchanged flags both occur
    return pages, seq


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] + "-" + f[2] for f in FORMS])
def sampled(request, capi, deck):
    """One matcher under the sampling and description, the sequence as frames of that sampling, and the restatement's BGR images."""
    name, s, fmt, desc = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    b = D.bps(desc[2])
    L, fb = R.make_layout(capi, fmt, w, h, b, -(-(2 * w if s == R.S422P else w * b) // 256) * 256, -(-h // 16) * 16)
    yuv = R.frames_to_yuv(seq, L, fb, desc, s)
    bgr = np.stack([R.to_bgr(f, w, h, L, desc, s) for f in yuv])
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    m.set_yuv_description(*desc)
    m.set_yuv_sampling(name)
    yield s, m, yuv, L, bgr, w, h
    m.close()


def test_the_restatements_images_are_close_to_the_source(sampled, deck):
    """(The forward transform of the test is sane: the bound tests/test_gpu_yuv_desc.py applies to 4:2:0, which keeps less chroma.)"""
    err = np.abs(sampled[4].astype(np.int32) - deck[1].astype(np.int32))
    assert np.median(err) <= 2


def test_match_frames_host_device_and_streaming(capi, sampled):
    import torch
    s, m, yuv, L, bgr, w, h = sampled
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
    c, _ = _code(capi, lambda: m.set_yuv_sampling("420"))         # a busy matcher refuses the setter, and the sampling stays
    assert c == 4 and m.yuv_sampling() == s
    got += [m.collect(t) for t in pend]
    assert _same(np.concatenate(got), want)


def test_changed_mask_kept_frames_and_gated_calls(capi, sampled):
    import torch
    s, m, yuv, L, bgr, w, h = sampled
    n, fs = yuv.shape
    ch, sim, last = m.changed_mask(bgr)
    assert ch.any() and not ch.all()
    kept_want = m.match_kept_frames([0, 3, 4])
    yc, ys, yl = m.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
    assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    yc2, ys2, yl2 = m.changed_mask_yuv420(yuv[3:], w, h, L, prev_small=yl)
    ch2, sim2, last2 = m.changed_mask(bgr[3:], prev_small=last)
    assert np.array_equal(yc2, ch2) and _same(ys2, sim2) and np.array_equal(yl2, last2)
    # the gate: two calls continuing one state, sync and submit / collect, and a state primed from one frame
    m.gate_reset()
    want = [m.match_changed_frames(bgr[:5]), m.match_changed_frames(bgr[5:])]
    want_small = m.gate_last_small()
    m.gate_reset()
    got = [m.match_changed_frames_yuv420(yuv[:5], w, h, L), m.match_changed_frames_yuv420(yuv[5:], w, h, L)]
    for g, wnt in zip(got, want):
        assert np.array_equal(g[0], wnt[0]) and _same(g[1], wnt[1]) and _same(g[2], wnt[2])
    assert np.array_equal(m.gate_last_small(), want_small)
    m.gate_reset()
    d = torch.from_numpy(yuv).cuda()
    tickets = [m.submit_changed_yuv420_dev(d.data_ptr(), 5, w, h, L, fs), m.submit_changed_yuv420_dev(d.data_ptr() + 5 * fs, n - 5, w, h, L, fs)]
    for t, wnt in zip(tickets, want):
        g = m.collect_changed(t)
        assert np.array_equal(g[0], wnt[0]) and _same(g[1], wnt[1]) and _same(g[2], wnt[2])
    m.gate_reset_from_frame(bgr[2])
    a = m.match_changed_frames(bgr[3:6])
    primed = m.gate_last_small()
    m.gate_reset_from_frame_yuv420(yuv[2], w, h, L)
    b = m.match_changed_frames_yuv420(yuv[3:6], w, h, L)
    assert np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]) and np.array_equal(m.gate_last_small(), primed)
    m.gate_reset()


def test_observe_frames_with_a_content_session(capi, sampled):
    s, m, yuv, L, bgr, w, h = sampled
    m.content_begin(24)
    m.observe_frames(bgr[:6])
    want = m.content_counts()
    m.content_begin(24)
    m.observe_frames_yuv420(yuv[:2], w, h, L)
    m.observe_frames_yuv420(yuv[2:6], w, h, L)
    got = m.content_counts()
    m.content_end()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] == 6


def test_group_of_two_members(capi, sampled, deck):
    s, m, yuv, L, bgr, w, h = sampled
    want = m.match_frames(bgr)
    ch, sim, last = m.changed_mask(bgr)
    m.gate_reset()
    gated = m.match_changed_frames(bgr)
    m.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    g.set_yuv_description(*m.yuv_description())
    g.set_yuv_sampling(s)
    assert g.yuv_sampling() == s
    assert _same(g.match_frames_yuv420(yuv, w, h, L), want)
    gc, gs, gl = g.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    got = g.match_changed_frames_yuv420(yuv, w, h, L)
    assert np.array_equal(got[0], gated[0]) and _same(got[1], gated[1]) and _same(got[2], gated[2])
    g.close()


def test_under_a_working_size_and_under_a_region(capi, sampled):
    s, m, yuv, L, bgr, w, h = sampled
    m.set_working_size(480, 270)
    try:
        want = m.match_frames(bgr[::2])
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), want)
        ch, sim, last = m.changed_mask(bgr[:6])
        yc, ys, yl = m.changed_mask_yuv420(yuv[:6], w, h, L)
        assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
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


def test_setting_it_ends_the_kept_frames_and_resets_the_gate(capi, sampled):
    s, m, yuv, L, bgr, w, h = sampled
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames_yuv420(yuv[:2], w, h, L)
    assert m.gate_last_small().ndim == 3
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    m.set_yuv_sampling(s)                                         # (the same value: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames_yuv420(yuv[1:3], w, h, L)
    assert ch[0]                                                  # the first gated frame after it is changed
    m.gate_reset()
