"""YUV transfer (include/slideo_amd.h "YUV transfer") on the GPU: the conversion tap under HLG and PQ is bit-exact against the numpy
restatement (tests/yuv_transfer_ref.py, over the integers of slideo_yuv_transfer_tables) — both ranges, both 10-bit depths, every
format of 4:2:0, 4:2:2 and 4:4:4, tight, pitched and skewed layouts, the sizes of the nearest kernels' tests —, SDR after a transfer
is the existing path, and every call form under a transfer returns exactly what its *_bgr8 twin returns on the restatement's images.
The tap takes one frame per call; the frame stride is exercised by the call forms here (n frames a call) and, two frames a record,
by the host build of the thread body in tests/test_yuv_transfer_abi.py.  Every test here fails without the feature: the setter does
not exist."""
import ctypes as C

import numpy as np
import pytest

import yuv_desc_ref as D
import yuv_transfer_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

# (id, format, (transfer, white_nits), range, depth): P010 under ("hlg", 0), yuv420p10le full range under ("pq", 100)
FORMS = [("p010-hlg", "nv12", (R.HLG, 0), R.LIMITED, R.D10_MSB),
         ("yuv420p10le-full-pq100", "i420", (R.PQ, 100), R.FULL, R.D10_LSB)]


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _same3(a, b):
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


def _sdr(x):
    """Back to the defaults, in an order every rule allows."""
    x.set_yuv_transfer("sdr")
    x.set_yuv_chroma("nearest")
    x.set_yuv_sampling("420")
    x.set_yuv_description()


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


# ---- 1. the tap ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampling,depth", [(s, d) for s in R.SAMPLINGS for d in R.DEPTHS], ids=lambda v: str(v))
def test_conversion_tap_bit_exact(capi, tap, sampling, depth):
    """Every format, size and layout; the transfer, the range and white_nits rotate over the cases, random frames (with 0, 64, 512,
    940, 960, 1023 sprinkled in and, for 10_LSB, containers above 1023) alternate with frames of those values alone."""
    _sdr(tap)
    tap.set_yuv_description("bt709", "limited", R.DEPTH_NAMES[depth])
    tap.set_yuv_sampling(R.SAMPLING_NAMES[sampling])
    k, tabs, seen = 0, {}, set()
    for fmt in R.FORMATS[sampling]:
        for w, h in R.sizes(sampling):
            for name, L, fb in R.layouts(capi, fmt, w, h, depth):
                transfer, rng, nits = R.pick(k)
                seen.add((transfer, rng))
                # the description's matrix is not consulted: it alternates and nothing changes
                tap.set_yuv_description(k % 2, rng, depth)
                tap.set_yuv_transfer(R.TRANSFER_NAMES[transfer], nits)
                assert tap.yuv_transfer() == (transfer, 203.0 if nits == 0 else float(nits))
                assert tap.yuv_sampling() == sampling and tap.yuv_description() == (k % 2, rng, depth)
                if (transfer, rng, nits) not in tabs:
                    tabs[(transfer, rng, nits)] = R.tables(capi, transfer, rng, nits)
                buf = R.special_frame(w, h, L, fb, depth, sampling) if k % 3 == 2 else R.random_frame(w, h, L, fb, depth, sampling, 1000 * depth + k)
                got = tap.yuv420_to_bgr(buf, w, h, L)
                want = R.to_bgr(buf, w, h, L, tabs[(transfer, rng, nits)], depth, sampling)
                assert np.array_equal(got, want), (transfer, rng, nits, fmt, w, h, name, np.argwhere(got != want)[:4])
                k += 1
    assert k >= len(R.FORMATS[sampling]) * len(R.sizes(sampling)) * 3 and len(seen) == 4
    # the size rules are unchanged: 4:2:0 needs even sides, 4:2:2 an even width
    if sampling != R.S444:
        fmt = R.FORMATS[sampling][0]
        L, fb = R.layouts(capi, fmt, 8, 4, depth)[0][1:]
        c, msg = _code(capi, lambda: tap.yuv420_to_bgr(np.zeros(fb, np.uint8), 7, 4, L))
        assert c == 5 and "even" in msg
    _sdr(tap)


def test_a_white_page_comes_out_white(capi, tap):
    """The use: an sRGB white and a mid grey, encoded as HLG / PQ at 203 nits, come back as themselves; read as SDR they do not."""
    img = np.zeros((4, 8, 3), np.uint8)
    img[:, :4], img[:, 4:] = 255, 128
    L, fb = capi.yuv420_layout("nv12", 8, 4, bytes_per_sample=2)
    for transfer in (R.HLG, R.PQ):
        yuv = R.frames_to_yuv(img[None], L, fb, transfer, R.LIMITED, R.D10_MSB, R.S420, 203)[0]
        _sdr(tap)
        tap.set_yuv_description("bt709", "limited", "10_msb")
        sdr = tap.yuv420_to_bgr(yuv, 8, 4, L)
        assert int(sdr[:, :4].max()) < 200
        tap.set_yuv_transfer(transfer, 203)
        got = tap.yuv420_to_bgr(yuv, 8, 4, L).astype(np.int32)
        assert np.abs(got - img).max() <= 2
    _sdr(tap)


def test_sdr_after_a_transfer_is_the_existing_path(capi, tap, deck):
    """After setting and clearing a transfer the tap, the verdicts and the changed mask equal a fresh matcher's."""
    pages, seq = deck
    fresh = capi.Matcher(small_cfg(capi))
    assert fresh.yuv_transfer() == (0, 0.0)
    _sdr(tap)
    tap.set_yuv_description("bt709", "full", "10_msb")
    tap.set_yuv_transfer("pq", 400)
    assert tap.yuv_transfer() == (2, 400.0)
    tap.set_yuv_transfer("sdr")
    assert tap.yuv_transfer() == (0, 0.0) and tap.yuv_description() == (D.BT709, D.FULL, D.D10_MSB)
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
    fresh.close()
    # verdicts and mask: one matcher before a transfer, under one, and after it
    n, h, w, _ = seq.shape
    desc = (D.BT709, D.LIMITED, D.D10_MSB)
    L, fb = capi.yuv420_layout("nv12", w, h, pitch=-(-w * 2 // 256) * 256, row_align=16, bytes_per_sample=2)
    yuv = D.frames_to_yuv(seq[:8], L, fb, desc)
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    m.set_yuv_description(*desc)
    want = m.match_frames_yuv420(yuv, w, h, L)
    wc, ws, wl = m.changed_mask_yuv420(yuv, w, h, L)
    assert (want["page_idx"] >= 0).mean() >= 0.5
    m.set_yuv_transfer("hlg")
    under = m.match_frames_yuv420(yuv, w, h, L)
    assert not _same(under, want)                                  # (the transfer does something on these frames)
    m.set_yuv_transfer("sdr")
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    gc, gs, gl = m.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(gc, wc) and _same(gs, ws) and np.array_equal(gl, wl)
    m.close()
    _sdr(tap)


def test_setter_refusals(capi, tap):
    _sdr(tap)
    # with 8-bit samples: refused, and the other way round
    c, msg = _code(capi, lambda: tap.set_yuv_transfer("hlg"))
    assert c == 5 and "SLIDEO_YUV_DEPTH_8" in msg and tap.yuv_transfer() == (0, 0.0)
    tap.set_yuv_description("bt709", "limited", "10_msb")
    tap.set_yuv_transfer("hlg", 300)
    c, msg = _code(capi, lambda: tap.set_yuv_description("bt709", "limited", 8))
    assert c == 5 and tap.yuv_description() == (1, 0, 1) and tap.yuv_transfer() == (1, 300.0)
    c, msg = _code(capi, lambda: tap.set_yuv_sampling("422_packed"))
    assert c == 5 and tap.yuv_sampling() == 0
    # with bilinear chroma: refused unless the sampling is 4:4:4, and the sampling cannot leave 4:4:4 then
    c, msg = _code(capi, lambda: tap.set_yuv_chroma("left"))
    assert c == 5 and "out of scope" in msg and tap.yuv_chroma() == 0
    tap.set_yuv_sampling("444")
    tap.set_yuv_chroma("left")
    c, msg = _code(capi, lambda: tap.set_yuv_sampling("420"))
    assert c == 5 and "out of scope" in msg and tap.yuv_sampling() == 2 and tap.yuv_transfer() == (1, 300.0)
    tap.set_yuv_chroma("nearest")
    tap.set_yuv_sampling("420")
    # bad values: INVALID_ARG, the state before stays
    for bad, nits in ((3, 0), (-1, 0), (1, float("nan")), (1, 0.5), (2, 20000), (0, 203)):
        c, msg = _code(capi, lambda: tap.set_yuv_transfer(bad, nits))
        assert c == 1 and "yuv transfer" in msg and tap.yuv_transfer() == (1, 300.0), (bad, nits)
    with pytest.raises(ValueError):
        tap.set_yuv_transfer("hdr10")
    assert tap.yuv_transfer() == (1, 300.0)
    _sdr(tap)
    # the group validates every member before it changes any
    g = capi.Group(small_cfg(capi), [0, 0])
    c, _ = _code(capi, lambda: g.set_yuv_transfer("pq"))
    assert c == 5 and g.yuv_transfer() == (0, 0.0)
    g.set_yuv_description("bt709", "full", "10_lsb")
    g.set_yuv_transfer("pq", 100)
    assert g.yuv_transfer() == (2, 100.0)
    c, _ = _code(capi, lambda: g.set_yuv_transfer(9, 0))
    assert c == 1 and g.yuv_transfer() == (2, 100.0)
    t, nn = C.c_int32(), C.c_float()
    member1 = C.c_void_p(capi.lib().slideo_group_member(g._h, 1))
    assert capi.lib().slideo_matcher_yuv_transfer(member1, C.byref(t), C.byref(nn)) == 0 and (t.value, nn.value) == (2, 100.0)
    g.set_yuv_sampling("422")
    g.set_yuv_description("bt601", "limited", "10_msb")
    assert g.yuv_transfer() == (2, 100.0) and g.yuv_sampling() == 1
    g.close()


# ---- 2. the call forms under a transfer --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.repeat(frames, 2, axis=0)                            # every frame twice: changed and unchanged flags both occur
    return pages, seq


def _frames_of(capi, seq, form):
    _, fmt, (transfer, nits), rng, depth = form
    n, h, w, _ = seq.shape
    L, fb = capi.yuv420_layout(fmt, w, h, pitch=-(-w * 2 // 256) * 256, row_align=16, bytes_per_sample=2)
    yuv = R.frames_to_yuv(seq, L, fb, transfer, rng, depth, R.S420, nits)
    return yuv, L, R.frames_to_bgr(yuv, w, h, L, R.tables(capi, transfer, rng, nits), depth, R.S420)


def _describe(x, form):
    _, fmt, (transfer, nits), rng, depth = form
    x.set_yuv_description("bt709", rng, depth)
    x.set_yuv_transfer(transfer, nits)


@pytest.fixture(scope="module", params=FORMS, ids=[f[0] for f in FORMS])
def under(request, capi, deck):
    """One matcher under the form's description and transfer, the sequence as HDR frames of that form, and the restatement's BGR
    images.  The matcher is its own twin: its BGR calls never look at the transfer."""
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


def test_the_restatements_images_are_close_to_the_source(under, deck):
    form, m, yuv, L, bgr, w, h = under
    err = np.abs(bgr.astype(np.int32) - deck[1].astype(np.int32))
    assert np.median(err) <= 1


def test_match_frames_host_device_and_streaming(capi, under):
    import torch
    form, m, yuv, L, bgr, w, h = under
    n, fs = yuv.shape
    want = m.match_frames(bgr)
    c_want = [m.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).mean() >= 0.5                  # the comparison is not over refusals
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    d = torch.from_numpy(yuv).cuda()
    before = d.clone()
    assert _same(m.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, fs), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of device frame %d" % i
    got, pend = [], []
    for i in range(0, n, 4):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_yuv420_dev(d.data_ptr() + i * fs, min(4, n - i), w, h, L, fs))
    c, _ = _code(capi, lambda: m.set_yuv_transfer("sdr"))         # a busy matcher refuses the setter, and the transfer stays
    assert c == 4 and m.yuv_transfer()[0] == form[2][0]
    got += [m.collect(t) for t in pend]
    assert _same(np.concatenate(got), want)
    torch.cuda.synchronize()
    assert torch.equal(d, before)                                 # the device frames are read, never written


def test_changed_mask_kept_frames_and_gated_calls(capi, under):
    import torch
    form, m, yuv, L, bgr, w, h = under
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


def test_observe_frames(capi, under):
    form, m, yuv, L, bgr, w, h = under
    m.levels_begin()
    m.observe_frames(bgr[:6])
    want = (m.levels_histogram().copy(), m.levels_info())
    m.levels_begin()
    m.observe_frames_yuv420(yuv[:2], w, h, L)
    m.observe_frames_yuv420(yuv[2:6], w, h, L)
    got = (m.levels_histogram().copy(), m.levels_info())
    m.levels_end()
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and want[0].any()


def test_group_of_two_members(capi, under, deck):
    form, m, yuv, L, bgr, w, h = under
    want = m.match_frames(bgr)
    ch, sim, last = m.changed_mask(bgr)
    m.gate_reset()
    gated = m.match_changed_frames(bgr)
    m.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    _describe(g, form)
    assert g.yuv_transfer()[0] == form[2][0]
    assert _same(g.match_frames_yuv420(yuv, w, h, L), want)
    gc, gs, gl = g.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same3(g.match_changed_frames_yuv420(yuv, w, h, L), gated)
    g.close()


def test_under_a_working_size_and_frame_levels(capi, under):
    form, m, yuv, L, bgr, w, h = under
    m.set_working_size(480, 270)
    try:
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), m.match_frames(bgr[::2]))
    finally:
        m.set_working_size(0, 0)
    m.set_frame_levels(capi.frame_levels_lut((10, 20, 30), (240, 230, 220)))
    try:
        assert m.yuv_transfer()[0] == form[2][0]
        assert _same(m.match_frames_yuv420(yuv[::2], w, h, L), m.match_frames(bgr[::2]))
    finally:
        m.set_frame_levels(None)
        m.gate_reset()


def test_setting_it_ends_the_kept_frames_and_resets_the_gate(capi, under):
    form, m, yuv, L, bgr, w, h = under
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames_yuv420(yuv[:2], w, h, L)
    assert m.gate_last_small().ndim == 3
    m.changed_mask_yuv420(yuv[:4], w, h, L)
    m.set_yuv_transfer(*form[2])                                  # (the same value: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames_yuv420(yuv[1:3], w, h, L)
    assert ch[0]                                                  # the first gated frame after it is changed
    m.gate_reset()
