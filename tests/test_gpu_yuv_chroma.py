"""YUV chroma filter (include/slideo_amd.h "YUV chroma filter") on the GPU: the conversion tap under the three bilinear filters is
bit-exact against the numpy restatement (tests/yuv_chroma_ref.py) — every format of 4:2:0, 4:2:2 and packed 4:2:2, its depths, tight,
pitched and skewed layouts, at the sizes where the stencil of yuv_chroma_to_bgr_kernel can go wrong —, the default filter is the
existing path, 4:4:4 ignores the filter, and every call form under a filter returns exactly what its *_bgr8 twin returns on the
restatement's images.  Every test here fails without the feature: the setter does not exist."""
import ctypes as C

import numpy as np
import pytest

import yuv420_ref as ref8
import yuv_chroma_ref as R
import yuv_desc_ref as D
import yuv_sampling_ref as S
from conftest import small_cfg

pytestmark = pytest.mark.gpu

# (id, sampling name, sampling, format, description, filter)
FORMS = [("nv12-left", "420", R.S420, "nv12", (D.BT601, D.LIMITED, D.D8), R.LEFT),
         ("p010-topleft", "420", R.S420, "nv12", (D.BT709, D.LIMITED, D.D10_MSB), R.TOPLEFT),
         ("nv16-10lsb-center", "422", R.S422, "nv16", (D.BT709, D.FULL, D.D10_LSB), R.CENTER),
         ("uyvy-left", "422_packed", R.S422P, "uyvy", (D.BT601, D.LIMITED, D.D8), R.LEFT)]


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _same3(a, b):
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


# ---- 1. the tap ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampling,depth", [(s, d) for s in R.SAMPLINGS for d in R.DEPTHS[s]], ids=lambda v: str(v))
def test_conversion_tap_bit_exact(capi, tap, sampling, depth):
    """Every size, format and layout under each of the three filters; the colour pair rotates."""
    tap.set_yuv_description()
    tap.set_yuv_sampling(S.SAMPLING_NAMES[sampling])
    k = 0
    for filt in R.FILTERS:
        tap.set_yuv_chroma(R.FILTER_NAMES[filt])
        assert tap.yuv_chroma() == filt and tap.yuv_sampling() == sampling
        for fmt in R.FORMATS[sampling]:
            for w, h in R.sizes(sampling):
                matrix, rng = D.PAIRS[k % 4]
                desc = (matrix, rng, depth)
                tap.set_yuv_description(*desc)
                assert tap.yuv_chroma() == filt                     # the description's setter leaves the filter alone
                for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                    k += 1
                    buf = R.random_frame(w, h, L, fb, depth, sampling, 1000 * depth + k)
                    got = tap.yuv420_to_bgr(buf, w, h, L)
                    want = R.to_bgr(buf, w, h, L, desc, sampling, filt)
                    assert np.array_equal(got, want), (desc, filt, fmt, w, h, name, np.argwhere(got != want)[:4])
    assert k >= 3 * len(R.FORMATS[sampling]) * len(R.sizes(sampling)) * 3          # three layouts at least, under three filters
    # the size rules are unchanged: 4:2:0 needs even sides, 4:2:2 an even width
    fmt = R.FORMATS[sampling][0]
    L, fb = R.layouts(capi, fmt, 8, 4, depth)[0][1:]
    c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(fb, np.uint8), 7, 4, L))
    assert c == 5 and "even" in msg
    if sampling == R.S420:
        c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(fb, np.uint8), 8, 3, L))
        assert c == 5 and "even" in msg
    tap.set_yuv_description()
    tap.set_yuv_sampling("420")
    tap.set_yuv_chroma("nearest")


def test_closed_form_through_the_kernel(capi, tap):
    """The 4x4 frame of the CPU test, grey luma: only the chroma planes differ between the filters, and the image is the
    restatement's of the hand-written U8 table."""
    L, fb = capi.yuv420_layout("i420", 4, 4)
    buf = np.full(fb, 128, np.uint8)
    buf[L.u_offset:L.u_offset + 4] = (0, 255, 0, 0)
    outs = {}
    for filt in (R.NEAREST,) + R.FILTERS:
        tap.set_yuv_chroma(filt)
        outs[filt] = tap.yuv420_to_bgr(buf, 4, 4, L)
        assert np.array_equal(outs[filt], R.to_bgr(buf, 4, 4, L, (0, 0, 0), R.S420, filt))
    assert len({o.tobytes() for o in outs.values()}) == 4
    tap.set_yuv_chroma("nearest")


def test_default_is_the_existing_path(capi, tap):
    """After setting and clearing a filter the tap over yuv_desc_ref's and yuv_sampling_ref's matrices equals a fresh matcher's."""
    fresh = capi.Matcher(small_cfg(capi))
    assert fresh.yuv_chroma() == 0
    tap.set_yuv_chroma("center")
    tap.set_yuv_sampling("422")
    tap.set_yuv_description("bt709", "full", "10_msb")
    assert (tap.yuv_chroma(), tap.yuv_sampling(), tap.yuv_description()) == (2, 1, (D.BT709, D.FULL, D.D10_MSB))
    tap.set_yuv_chroma("nearest")
    assert (tap.yuv_chroma(), tap.yuv_sampling(), tap.yuv_description()) == (0, 1, (D.BT709, D.FULL, D.D10_MSB))
    tap.set_yuv_sampling("420")
    tap.set_yuv_description()
    k = 0
    for depth in D.DEPTHS:
        for w, h in D.SIZES:
            for fmt in D.FORMATS:
                for name, L, fb in D.layouts(capi, fmt, w, h, depth):
                    m_, r_ = D.PAIRS[k % 4]
                    k += 1
                    for x in (tap, fresh):
                        x.set_yuv_description(m_, r_, depth)
                    buf = D.random_frame(w, h, L, fb, depth, w + h + k)
                    got = tap.yuv420_to_bgr(buf, w, h, L)
                    assert np.array_equal(got, fresh.yuv420_to_bgr(buf, w, h, L)), (fmt, w, h, name)
                    assert np.array_equal(got, D.to_bgr(buf, w, h, L, (m_, r_, depth)))
                    if (m_, r_, depth) == (0, 0, 0):
                        assert np.array_equal(got, ref8.to_bgr(buf, w, h, L))
    for s in S.SAMPLINGS:
        for x in (tap, fresh):
            x.set_yuv_description()
            x.set_yuv_sampling(s)
        for depth in S.DEPTHS[s]:
            for w, h in S.sizes(s):
                for fmt in S.FORMATS[s]:
                    for name, L, fb in S.layouts(capi, fmt, w, h, depth):
                        m_, r_ = D.PAIRS[k % 4]
                        k += 1
                        for x in (tap, fresh):
                            x.set_yuv_description(m_, r_, depth)
                        buf = S.random_frame(w, h, L, fb, depth, s, k)
                        got = tap.yuv420_to_bgr(buf, w, h, L)
                        assert np.array_equal(got, fresh.yuv420_to_bgr(buf, w, h, L)), (s, fmt, w, h, name)
                        assert np.array_equal(got, S.to_bgr(buf, w, h, L, (m_, r_, depth), s))
    tap.set_yuv_description()
    tap.set_yuv_sampling("420")
    fresh.close()


def test_444_ignores_the_filter(capi, tap):
    tap.set_yuv_sampling("444")
    k = 0
    for depth in S.DEPTHS[S.S444]:
        tap.set_yuv_description(D.BT709, D.LIMITED, depth)
        for w, h in S.sizes(S.S444):
            for fmt in S.FORMATS[S.S444]:
                for name, L, fb in S.layouts(capi, fmt, w, h, depth):
                    k += 1
                    buf = S.random_frame(w, h, L, fb, depth, S.S444, k)
                    tap.set_yuv_chroma("nearest")
                    want = tap.yuv420_to_bgr(buf, w, h, L)
                    tap.set_yuv_chroma(R.FILTER_NAMES[R.FILTERS[k % 3]])
                    assert tap.yuv_chroma() == R.FILTERS[k % 3]
                    assert np.array_equal(tap.yuv420_to_bgr(buf, w, h, L), want), (fmt, w, h, name)
    tap.set_yuv_chroma("nearest")
    tap.set_yuv_description()
    tap.set_yuv_sampling("420")


def test_setter_refusals(capi, tap):
    tap.set_yuv_chroma("left")
    for bad in (4, -1, 16):
        c, msg = _code(capi, lambda: tap.set_yuv_chroma(bad))
        assert c == 1 and "yuv chroma filter" in msg and tap.yuv_chroma() == 1     # the state before stays
    with pytest.raises(ValueError):
        tap.set_yuv_chroma("centre")
    assert tap.yuv_chroma() == 1
    tap.set_yuv_chroma("nearest")
    # the group validates every member before it changes any
    g = capi.Group(small_cfg(capi), [0, 0])
    g.set_yuv_chroma("topleft")
    assert g.yuv_chroma() == 3
    c, _ = _code(capi, lambda: g.set_yuv_chroma(9))
    assert c == 1 and g.yuv_chroma() == 3
    v = C.c_int32()
    member1 = C.c_void_p(capi.lib().slideo_group_member(g._h, 1))
    assert capi.lib().slideo_matcher_yuv_chroma(member1, C.byref(v)) == 0 and v.value == 3
    g.set_yuv_sampling("422")
    g.set_yuv_description("bt709", "full", 8)
    assert g.yuv_chroma() == 3 and g.yuv_sampling() == 1
    g.close()


# ---- 2. the call forms under a filter ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.repeat(frames, 2, axis=0)                            # every frame twice: changed and unchanged flags both occur
    return pages, seq


def _frames_of(capi, seq, form):
    _, name, s, fmt, desc, filt = form
    n, h, w, _ = seq.shape
    b = D.bps(desc[2])
    if s == R.S420:
        L, fb = capi.yuv420_layout(fmt, w, h, pitch=-(-w * b // 256) * 256, row_align=16, bytes_per_sample=b)
    else:
        L, fb = S.make_layout(capi, fmt, w, h, b, -(-(2 * w if s == R.S422P else w * b) // 256) * 256, -(-h // 16) * 16)
    yuv = R.frames_to_yuv(seq, L, fb, desc, s)
    return yuv, L, R.frames_to_bgr(yuv, w, h, L, desc, s, filt)


def _describe(x, form):
    _, name, s, fmt, desc, filt = form
    x.set_yuv_description(*desc)
    x.set_yuv_sampling(name)
    x.set_yuv_chroma(filt)


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def filtered(request, capi, deck):
    """One matcher under the form's description, sampling and filter, the sequence as frames of that form, and the restatement's
    BGR images.  The matcher is its own twin: its BGR calls never look at the filter."""
    form = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    yuv, L, bgr = _frames_of(capi, seq, form)
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    _describe(m, form)                                            # after finalize
    yield form, m, yuv, L, bgr, w, h
    m.close()


def test_the_restatements_images_are_close_to_the_source_and_differ_from_nearest(filtered, deck):
    form, m, yuv, L, bgr, w, h = filtered
    err = np.abs(bgr.astype(np.int32) - deck[1].astype(np.int32))
    assert np.median(err) <= 2
    near = R.to_bgr(yuv[0], w, h, L, form[4], form[2], R.NEAREST)
    assert not np.array_equal(near, bgr[0])                       # (the filter does something on these frames)


def test_match_frames_host_device_and_streaming(capi, filtered):
    import torch
    form, m, yuv, L, bgr, w, h = filtered
    n, fs = yuv.shape
    want = m.match_frames(bgr)
    c_want = [m.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).mean() >= 0.5
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    d = torch.from_numpy(yuv).cuda()
    before = d.clone()
    assert _same(m.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, fs), want)
    got, pend = [], []
    for i in range(0, n, 4):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_yuv420_dev(d.data_ptr() + i * fs, min(4, n - i), w, h, L, fs))
    c, _ = _code(capi, lambda: m.set_yuv_chroma("nearest"))       # a busy matcher refuses the setter, and the filter stays
    assert c == 4 and m.yuv_chroma() == form[5]
    got += [m.collect(t) for t in pend]
    assert _same(np.concatenate(got), want)
    torch.cuda.synchronize()
    assert torch.equal(d, before)                                 # the device frames are read, never written


def test_changed_mask_kept_frames_and_gated_calls(capi, filtered):
    import torch
    form, m, yuv, L, bgr, w, h = filtered
    n, fs = yuv.shape
    ch, sim, last = m.changed_mask(bgr)
    assert ch.any() and not ch.all()
    kept_want = m.match_kept_frames([0, 3, 4])
    yc, ys, yl = m.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
    assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    # the gate: two calls continuing one state, sync and submit / collect, and a state primed from one frame
    m.gate_reset()
    want = [m.match_changed_frames(bgr[:5]), m.match_changed_frames(bgr[5:])]
    want_small = m.gate_last_small()
    m.gate_reset()
    got = [m.match_changed_frames_yuv420(yuv[:5], w, h, L), m.match_changed_frames_yuv420(yuv[5:], w, h, L)]
    assert _same3(got[0], want[0]) and _same3(got[1], want[1])
    assert np.array_equal(m.gate_last_small(), want_small)
    m.gate_reset()
    d = torch.from_numpy(yuv).cuda()
    before = d.clone()
    tickets = [m.submit_changed_yuv420_dev(d.data_ptr(), 5, w, h, L, fs), m.submit_changed_yuv420_dev(d.data_ptr() + 5 * fs, n - 5, w, h, L, fs)]
    for t, wnt in zip(tickets, want):
        assert _same3(m.collect_changed(t), wnt)
    m.gate_reset()
    got = [m.match_changed_frames_yuv420_dev(d.data_ptr(), 5, w, h, L, fs), m.match_changed_frames_yuv420_dev(d.data_ptr() + 5 * fs, n - 5, w, h, L, fs)]
    assert _same3(got[0], want[0]) and _same3(got[1], want[1])
    m.gate_reset_from_frame(bgr[2])
    a = m.match_changed_frames(bgr[3:6])
    primed = m.gate_last_small()
    m.gate_reset_from_frame_yuv420(yuv[2], w, h, L)
    assert _same3(m.match_changed_frames_yuv420(yuv[3:6], w, h, L), a) and np.array_equal(m.gate_last_small(), primed)
    m.gate_reset_from_frame_yuv420_dev(d.data_ptr() + 2 * fs, w, h, L)
    assert _same3(m.match_changed_frames_yuv420_dev(d.data_ptr() + 3 * fs, 3, w, h, L, fs), a)
    m.gate_reset()
    torch.cuda.synchronize()
    assert torch.equal(d, before)


def test_observe_frames_with_the_three_sessions(capi, filtered):
    import torch
    form, m, yuv, L, bgr, w, h = filtered
    n, fs = yuv.shape

    def begin():
        m.activity_begin(12)
        m.content_begin(24)
        m.levels_begin()

    begin()
    m.observe_frames(bgr[:2])
    m.observe_frames(bgr[2:10])
    want = (m.activity_counts(), m.content_counts(), m.levels_histogram().copy(), m.levels_info())
    begin()
    m.observe_frames_yuv420(yuv[:2], w, h, L)
    m.observe_frames_yuv420(yuv[2:7], w, h, L)
    d = torch.from_numpy(yuv).cuda()
    before = d.clone()
    m.observe_frames_yuv420_dev(d.data_ptr() + 7 * fs, 3, w, h, L, fs)
    got = (m.activity_counts(), m.content_counts(), m.levels_histogram().copy(), m.levels_info())
    m.activity_end(); m.content_end(); m.levels_end()
    assert np.array_equal(got[0][0], want[0][0]) and got[0][1] == want[0][1] == 9 and want[0][0].any()
    assert np.array_equal(got[1][0], want[1][0]) and got[1][1] == want[1][1] == 10
    assert np.array_equal(got[2], want[2]) and got[3] == want[3] and want[2].any()
    torch.cuda.synchronize()
    assert torch.equal(d, before)


def test_group_of_two_members(capi, filtered, deck):
    form, m, yuv, L, bgr, w, h = filtered
    want = m.match_frames(bgr)
    ch, sim, last = m.changed_mask(bgr)
    m.gate_reset()
    gated = m.match_changed_frames(bgr)
    m.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    _describe(g, form)
    assert g.yuv_chroma() == form[5] and g.yuv_sampling() == form[2]
    assert _same(g.match_frames_yuv420(yuv, w, h, L), want)
    gc, gs, gl = g.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same3(g.match_changed_frames_yuv420(yuv, w, h, L), gated)
    g.close()


def test_under_a_working_size_a_region_and_frame_levels(capi, filtered):
    form, m, yuv, L, bgr, w, h = filtered
    m.set_working_size(480, 270)
    try:
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), m.match_frames(bgr[::2]))
        ch, sim, last = m.changed_mask(bgr[:6])
        yc, ys, yl = m.changed_mask_yuv420(yuv[:6], w, h, L)
        assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
    finally:
        m.set_working_size(0, 0)
    m.set_frame_region(w, h, [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)], 480, 270)
    try:
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), m.match_frames(bgr[::2]))
        m.gate_reset()
        a = m.match_changed_frames(bgr[:6])
        m.gate_reset()
        assert _same3(m.match_changed_frames_yuv420(yuv[:6], w, h, L), a)
    finally:
        m.clear_frame_region()
        m.gate_reset()
    m.set_frame_levels(capi.frame_levels_lut((10, 20, 30), (240, 230, 220)))
    try:
        assert m.yuv_chroma() == form[5]
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), m.match_frames(bgr[::2]))
        m.gate_reset()
        a = m.match_changed_frames(bgr[:6])
        m.gate_reset()
        assert _same3(m.match_changed_frames_yuv420(yuv[:6], w, h, L), a)
    finally:
        m.set_frame_levels(None)
        m.gate_reset()


def test_sift_mode(capi, deck):
    form = FORMS[0]
    pages, seq = deck
    sel = seq[::3]
    n, h, w, _ = sel.shape
    yuv, L, bgr = _frames_of(capi, sel, form)
    m = capi.Matcher(small_cfg(capi))
    m.use_sift(capi.sift_config(nfeatures=300), 0.0)
    m.add_pages(list(pages))
    m.finalize()
    _describe(m, form)
    want = m.match_frames(bgr)
    c_want = [m.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).any()
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i])
    m.close()


def test_setting_it_ends_the_kept_frames_and_resets_the_gate(capi, filtered):
    form, m, yuv, L, bgr, w, h = filtered
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames_yuv420(yuv[:2], w, h, L)
    assert m.gate_last_small().ndim == 3
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    m.set_yuv_chroma(form[5])                                     # (the same value: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames_yuv420(yuv[1:3], w, h, L)
    assert ch[0]                                                  # the first gated frame after it is changed
    m.gate_reset()
