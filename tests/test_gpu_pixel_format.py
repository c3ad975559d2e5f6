"""Frame pixel format (include/slideo_amd.h "Frame pixel format") on the GPU: the conversion tap under all eight non-default formats
is bit-exact against the numpy restatement (tests/pixel_format_ref.py) over sizes and layouts that make every wide load of
pixels_to_bgr_kernel and its fallback run; the default format is the existing path; every call form under a format returns exactly
what the same call under the default returns on the restated image; the refusals; and the two doors do not look at each other's
settings.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import pixel_format_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

FORMS = ["rgb", "argb", "planar_gbr"]                             # one per kernel instance: PACKED3, PACKED4, PLANAR


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _same3(a, b):
    """(changed, similarity, verdicts) of two gated calls."""
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


# ---- 1. the tap, bit-exact ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", R.NON_DEFAULT)
def test_conversion_tap_bit_exact(capi, tap, fmt):
    tap.set_pixel_format(fmt)
    assert tap.pixel_format() == R.FORMATS[fmt]
    rng = np.random.default_rng(R.FORMATS[fmt])
    for w, h in R.sizes():
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for k, (name, stride) in enumerate(R.layouts(fmt, w, h)):
            buf = R.pack(img, fmt, stride, seed=w * 31 + h + k)
            assert np.array_equal(R.to_bgr(buf, w, h, stride, fmt), img)
            got = tap.pixels_to_bgr((buf, w, h), stride=stride)
            assert np.array_equal(got, img), (fmt, w, h, name, np.argwhere(got != img)[:4])
        # the array form of the Python method: the format's shape, tight
        tight = R.pack(img, fmt, seed=7)
        assert np.array_equal(tap.pixels_to_bgr(R.as_array(tight, fmt, w, h)), img)
    tap.set_pixel_format("bgr")


# ---- 2. the default is the existing path ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.ascontiguousarray(np.repeat(frames, 2, axis=0))      # every frame twice: changed and unchanged flags both occur
    return pages, seq


def _matcher(capi, pages, fmt=None, sift=None):
    m = capi.Matcher(small_cfg(capi))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if fmt is not None:
        m.set_pixel_format(fmt)
    return m


def test_default_is_the_existing_path(capi, deck):
    import torch
    pages, seq = deck
    n, h, w, _ = seq.shape
    fresh, m = _matcher(capi, pages), _matcher(capi, pages)
    m.set_pixel_format("rgba")
    assert m.pixel_format() == 3
    m.set_pixel_format("bgr")
    assert m.pixel_format() == 0 and fresh.pixel_format() == 0
    # the tap is the identity copy, row by row to stride 3w
    rng = np.random.default_rng(5)
    for tw, th, stride in ((7, 5, 21), (7, 5, 32), (64, 36, 200)):
        buf = rng.integers(0, 256, th * stride, dtype=np.uint8)
        want = np.stack([buf[y * stride: y * stride + 3 * tw].reshape(tw, 3) for y in range(th)])
        assert np.array_equal(m.pixels_to_bgr((buf, tw, th), stride=stride), want)
    assert np.array_equal(m.pixels_to_bgr(seq[0]), seq[0])
    want = fresh.match_frames(seq)
    assert _same(m.match_frames(seq), want)
    d = torch.from_numpy(seq).cuda()
    assert _same(m.match_frames_dev(d.data_ptr(), n, w, h), fresh.match_frames_dev(d.data_ptr(), n, w, h))
    assert _same(m.match_frames_dev(d.data_ptr(), n, w, h), want)
    for x in (m, fresh):
        x.gate_reset()
    assert _same3(m.match_changed_frames(seq), fresh.match_changed_frames(seq))
    assert np.array_equal(m.gate_last_small(), fresh.gate_last_small())
    m.close(); fresh.close()


# ---- 3. every call form under a format equals its default twin on the restated image ------------------------------------------------

@pytest.fixture(scope="module", params=FORMS)
def pair(request, capi, deck):
    """A matcher under the format, a matcher under the default, the sequence as tight frames of the format (flat and in the
    format's array shape) and the restatement's BGR images of those frames."""
    fmt = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    flat = np.stack([R.pack(seq[i], fmt, seed=i) for i in range(n)])
    bgr = np.stack([R.to_bgr(flat[i], w, h, w * R.info(fmt)[0], fmt) for i in range(n)])
    assert np.array_equal(bgr, seq)
    m, ref = _matcher(capi, pages, fmt), _matcher(capi, pages)
    yield fmt, m, ref, R.as_array(flat, fmt, w, h), bgr, w, h
    m.close(); ref.close()


def _device_frames(fmt, bgr, ofs, pitch_extra=0, slack=0):
    """The images as device frames of fmt, rows pitch_extra bytes beyond tight, frames `slack` bytes beyond the span apart, the first
    byte `ofs` bytes past the allocation's (256-byte aligned) base -> (tensor kept alive, pointer, stride, frame stride)."""
    import torch
    n, h, w, _ = bgr.shape
    stride = w * R.info(fmt)[0] + pitch_extra
    fs = R.span(fmt, w, h, stride) + slack
    host = np.concatenate([R.pack(bgr[i], fmt, stride, fs, seed=50 + i) for i in range(n)])
    t = torch.empty(ofs + host.size, dtype=torch.uint8, device="cuda")
    t[ofs:].copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    return t, t.data_ptr() + ofs, stride, fs


def test_match_frames_host_device_and_streaming(capi, pair):
    fmt, m, ref, frames, bgr, w, h = pair
    n = len(bgr)
    want = ref.match_frames(bgr)
    c_want = [ref.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).mean() >= 0.5
    assert _same(m.match_frames(frames), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    for ofs, extra, slack in ((0, 0, 0), (1, 0, 0), (4, 8, 12)):
        t, p, stride, fs = _device_frames(fmt, bgr, ofs, extra, slack)
        assert _same(m.match_frames_dev(p, n, w, h, stride, fs), want), (ofs, extra, slack)
        for i in range(n):
            assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d from a device base offset of %d" % (i, ofs)
    t, p, stride, fs = _device_frames(fmt, bgr, 0)
    assert _same(m.match_frames_dev(p, n, w, h), want)           # the default strides follow the format
    got, pend = [], []
    for i in range(0, n, 4):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_dev(p + i * fs, min(4, n - i), w, h))
    c, _ = _code(capi, lambda: m.set_pixel_format("bgr"))         # a busy matcher refuses the setter, and the format stays
    assert c == 4 and m.pixel_format() == R.FORMATS[fmt]
    got += [m.collect(t_) for t_ in pend]
    assert _same(np.concatenate(got), want)


def test_changed_mask_and_kept_frames(capi, pair):
    fmt, m, ref, frames, bgr, w, h = pair
    ch, sim, last = ref.changed_mask(bgr)
    assert ch.any() and not ch.all()
    kept_want = ref.match_kept_frames([0, 3, 4])
    gc, gs, gl = m.changed_mask(frames)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    gc2, gs2, gl2 = m.changed_mask(frames[3:], prev_small=gl)
    ch2, sim2, last2 = ref.changed_mask(bgr[3:], prev_small=last)
    assert np.array_equal(gc2, ch2) and _same(gs2, sim2) and np.array_equal(gl2, last2)


@pytest.mark.parametrize("gate", ["previous", "anchor_settle"])
def test_gated_calls(capi, pair, gate):
    fmt, m, ref, frames, bgr, w, h = pair
    n = len(bgr)
    for x in (m, ref):
        if gate == "anchor_settle":
            x.set_gate_reference("anchor")
            x.set_gate_settle(0.99, 2)
        x.gate_reset()
    try:
        # two calls continuing one state: host, device, submit / collect; then a state primed from one frame
        want = [ref.match_changed_frames(bgr[:5]), ref.match_changed_frames(bgr[5:])]
        want_small = ref.gate_last_small()
        got = [m.match_changed_frames(frames[:5]), m.match_changed_frames(frames[5:])]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1])
        assert np.array_equal(m.gate_last_small(), want_small)
        assert m.gate_state_export() == ref.gate_state_export()
        t, p, stride, fs = _device_frames(fmt, bgr, 4, 4, 8)
        m.gate_reset()
        got = [m.match_changed_frames_dev(p, 5, w, h, stride, fs), m.match_changed_frames_dev(p + 5 * fs, n - 5, w, h, stride, fs)]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1]) and m.gate_state_export() == ref.gate_state_export()
        m.gate_reset()
        tickets = [m.submit_changed_dev(p, 5, w, h, stride, fs), m.submit_changed_dev(p + 5 * fs, n - 5, w, h, stride, fs)]
        for tk, wnt in zip(tickets, want):
            assert _same3(m.collect_changed(tk), wnt)
        assert m.gate_state_export() == ref.gate_state_export()
        ref.gate_reset_from_frame(bgr[2])
        a = ref.match_changed_frames(bgr[3:6])
        m.gate_reset_from_frame(frames[2])
        assert m.gate_state_export() != b"" and _same3(m.match_changed_frames(frames[3:6]), a)
        assert np.array_equal(m.gate_last_small(), ref.gate_last_small())
        m.gate_reset_from_frame_dev(p + 2 * fs, w, h, stride)
        assert _same3(m.match_changed_frames_dev(p + 3 * fs, 3, w, h, stride, fs), a)
        assert m.gate_state_export() == ref.gate_state_export()
    finally:
        for x in (m, ref):
            x.set_gate_settle(0, 0)
            x.set_gate_reference("previous")
            x.gate_reset()


def test_observe_frames_activity_and_content(capi, pair):
    fmt, m, ref, frames, bgr, w, h = pair
    for x, f in ((ref, bgr), (m, frames)):
        x.activity_begin(12)
        x.content_begin(24)
        x.observe_frames(f[:2])
        x.observe_frames(f[2:7])
    t, p, stride, fs = _device_frames(fmt, bgr, 1, 0, 3)
    m.observe_frames_dev(p + 7 * fs, 3, w, h, stride, fs)
    ref.observe_frames(bgr[7:10])
    a, b = m.activity_counts(), ref.activity_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 9 and b[0].any()
    a, b = m.content_counts(), ref.content_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 10
    for x in (m, ref):
        x.activity_end()
        x.content_end()


def test_group_of_two_members(capi, pair, deck):
    fmt, m, ref, frames, bgr, w, h = pair
    want = ref.match_frames(bgr)
    ch, sim, last = ref.changed_mask(bgr)
    kept = ref.match_kept_frames([1, 2, 9])
    ref.gate_reset()
    gated = ref.match_changed_frames(bgr)
    ref.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    g.set_pixel_format(fmt)
    assert g.pixel_format() == R.FORMATS[fmt]
    assert _same(g.match_frames(frames), want)
    gc, gs, gl = g.changed_mask(frames)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(g.match_kept_frames([1, 2, 9]), kept)
    assert _same3(g.match_changed_frames(frames), gated)
    # the group's setter validates every member before it changes any
    c, _ = _code(capi, lambda: g.set_pixel_format(9))
    assert c == 1 and g.pixel_format() == R.FORMATS[fmt]
    v = C.c_int32()
    assert capi.lib().slideo_matcher_pixel_format(C.c_void_p(capi.lib().slideo_group_member(g._h, 1)), C.byref(v)) == 0 and v.value == R.FORMATS[fmt]
    g.close()


def test_under_a_working_size_a_region_and_a_gate_mask(capi, pair):
    fmt, m, ref, frames, bgr, w, h = pair
    t, p, stride, fs = _device_frames(fmt, bgr, 0, 4, 0)
    for x in (m, ref):
        x.set_working_size(480, 270)
    try:
        want = ref.match_frames(bgr[::2])
        assert _same(m.match_frames(frames[::2]), want)
        assert _same(m.match_frames_dev(p, 6, w, h, stride, fs), ref.match_frames(bgr[:6]))
        ch, sim, last = ref.changed_mask(bgr[:6])
        gc, gs, gl = m.changed_mask(frames[:6])
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        for x in (m, ref):
            x.set_working_size(0, 0)
    for x in (m, ref):
        x.set_frame_region(w, h, [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)], 480, 270)
    try:
        assert _same(m.match_frames(frames[::2]), ref.match_frames(bgr[::2]))
        for x in (m, ref):
            x.gate_reset()
        a = ref.match_changed_frames(bgr[:6])
        assert _same3(m.match_changed_frames(frames[:6]), a)
        m.gate_reset()
        assert _same3(m.match_changed_frames_dev(p, 6, w, h, stride, fs), a)
    finally:
        for x in (m, ref):
            x.clear_frame_region()
            x.gate_reset()
    mask = np.full((h, w), 255, np.uint8)
    mask[: h // 3, w // 2:] = 0
    for x in (m, ref):
        x.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        x.set_frame_mask(mask)
        x.gate_reset()
    try:
        a = ref.match_changed_frames(bgr)
        assert _same3(m.match_changed_frames(frames), a)
        for i in range(int(a[0].sum())):
            assert _same(m.last_candidates(i), ref.last_candidates(i))
        ch, sim, last = ref.changed_mask(bgr[:6])
        gc, gs, gl = m.changed_mask(frames[:6])
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        for x in (m, ref):
            x.set_frame_mask(None)
            x.set_frame_mask_scope(capi.MASK_DETECT)
            x.gate_reset()


def test_sift_mode(capi, deck):
    pages, seq = deck
    n, h, w, _ = seq.shape
    sift = (capi.sift_config(nfeatures=300), 0.0)
    m, ref = _matcher(capi, pages, "rgb", sift), _matcher(capi, pages, None, sift)
    sel = seq[::3]
    frames = np.stack([R.as_array(R.pack(f, "rgb", seed=3), "rgb", w, h) for f in sel])
    want = ref.match_frames(sel)
    assert (want["page_idx"] >= 0).any()
    assert _same(m.match_frames(frames), want)
    for i in range(len(sel)):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    m.close(); ref.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(capi, pair):
    fmt, m, ref, frames, bgr, w, h = pair
    n = len(bgr)
    bpp, planes = R.info(fmt)
    cname = R.C_NAMES[R.FORMATS[fmt]]
    L = capi.lib()
    out = np.zeros(n, capi.VERDICT_DTYPE)
    flat = np.ascontiguousarray(frames).reshape(n, -1)
    fs = flat.shape[1]
    args = lambda stride, fstride: (m._h, n, flat.ctypes.data_as(C.c_void_p), w, h, stride, C.c_int64(fstride), out.ctypes.data_as(C.c_void_p))
    # stride < bpp * width, the format named
    assert L.slideo_match_frames_bgr8(*args(bpp * w - 1, fs)) == 1
    msg = L.slideo_last_error(m._h).decode()
    assert "stride_bytes" in msg and cname in msg
    # a frame stride that does not cover the span (planar: one plane only)
    assert L.slideo_match_frames_bgr8(*args(bpp * w, w * h if planes == 3 else fs - 1)) == 1
    msg = L.slideo_last_error(m._h).decode()
    assert "frame_stride" in msg and cname in msg and (planes == 1 or "three planes" in msg)
    assert L.slideo_match_frames_bgr8(*args(bpp * w, fs)) == 0
    # the Python methods name the expected shape
    with pytest.raises(ValueError) as e:
        m.match_frames(np.zeros((2, h, w, 5), np.uint8))
    assert fmt in str(e.value) and ("[n, 3, h, w]" if planes == 3 else "[n, h, w, %d]" % bpp) in str(e.value)
    # an enum value of 9: refused, the state before kept
    c, msg = _code(capi, lambda: m.set_pixel_format(9))
    assert c == 1 and "pixel format" in msg and m.pixel_format() == R.FORMATS[fmt]
    assert _code(capi, lambda: m.set_pixel_format("grey"))[0] == 1
    # setting it ends the kept frames and resets the gate state to "none"
    m.changed_mask(frames[:4])
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames(frames[:2])
    assert m.gate_last_small().ndim == 3
    m.changed_mask(frames[:4])
    m.set_pixel_format(fmt)                                       # (the same value: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames(frames[1:3])
    assert ch[0]                                                  # the first gated frame after it is changed
    m.gate_reset()


# ---- 5. independence of the two doors -------------------------------------------------------------------------------------------------

def test_the_doors_do_not_look_at_each_others_settings(capi, deck):
    pages, seq = deck
    n, h, w, _ = seq.shape
    sel = seq[:6]
    m, ref = _matcher(capi, pages), _matcher(capi, pages)
    # under rgba a _yuv420 call returns what it returns under bgr
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = np.random.default_rng(1).integers(16, 236, (3, fb), dtype=np.uint8)
    want_img = ref.yuv420_to_bgr(yuv[0], w, h, L)
    want = ref.match_frames_yuv420(yuv, w, h, L)
    m.set_pixel_format("rgba")
    assert np.array_equal(m.yuv420_to_bgr(yuv[0], w, h, L), want_img)
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    ref.gate_reset(); m.gate_reset()
    assert _same3(m.match_changed_frames_yuv420(yuv, w, h, L), ref.match_changed_frames_yuv420(yuv, w, h, L))
    # under the sampling 444 and a non-default description a _bgr8 call under rgb still equals its twin
    m.set_yuv_sampling("444")
    m.set_yuv_description("bt709", "full", "10_msb")
    m.set_pixel_format("rgb")
    frames = np.stack([R.as_array(R.pack(f, "rgb", seed=9), "rgb", w, h) for f in sel])
    assert _same(m.match_frames(frames), ref.match_frames(sel))
    ref.gate_reset(); m.gate_reset()
    assert _same3(m.match_changed_frames(frames), ref.match_changed_frames(sel))
    assert m.yuv_sampling() == 2 and m.yuv_description() == (1, 1, 1) and m.pixel_format() == 1
    m.close(); ref.close()
