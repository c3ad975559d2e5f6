"""Frame activity map (include/slideo_amd.h "Frame activity map") on the GPU: the counts through the tap against ONE numpy
restatement (tests/activity_ref.py) on every path frames arrive by, the observed image against the images the taps return, the mask
read-out, the rules, and the use the feature is for: a mask learnt from frames with a moving inset equals the hand-made one."""
import ctypes as C

import numpy as np
import pytest

import activity_ref as A
import yuv420_ref as yref
import yuv_desc_ref as dref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

SIZES = [(640, 360), (349, 347), (402, 300), (403, 33)]             # aw % 4 in {0, 1, 2, 3}
N, DELTA = 23, 24


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


@pytest.fixture(scope="module")
def bare(capi):
    """A matcher with no pages: observing needs none."""
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


def _counts_of(m, observe, delta=DELTA):
    m.activity_begin(delta)
    observe()
    return m.activity_counts()


def _same(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), "%s: %d counts differ" % (what, int((got[0] != want[0]).sum()))


# ---- 1. counts equal the restatement, on every path --------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_counts_equal_the_restatement(capi, bare, w, h):
    import torch
    m, L = bare, capi.lib()
    frames = A.moving_frames(N, h, w, w * 7 + h)
    want = A.counts(frames, DELTA)
    assert want[1] == N - 1 and 0 < int((want[0] > 0).sum()) < w * h
    whole = _counts_of(m, lambda: m.observe_frames(frames))          # one observation of everything at once
    _same(whole, want, "host, tight")
    assert m.activity_info() == {"aw": w, "ah": h, "pairs": N - 1, "delta": DELTA}

    def padded(stride, ofs):
        buf = np.full(ofs + N * h * stride, 0x5A, np.uint8)
        rows = np.lib.stride_tricks.as_strided(buf[ofs:], (N, h, w * 3), (h * stride, stride, 1))
        rows[:] = frames.reshape(N, h, w * 3)
        return buf
    odd = 3 * w + 5 if (3 * w + 5) % 4 else 3 * w + 6
    buf = padded(odd, 0)
    _same(_counts_of(m, lambda: m._check(L.slideo_matcher_observe_frames_bgr8(m._h, N, buf.ctypes.data, w, h, odd, C.c_int64(h * odd)))), want,
          "host, padded stride")
    # device frames at every base alignment, tight and with an odd stride (read in place)
    for ofs in range(4):
        for stride in (3 * w, odd):
            d = torch.from_numpy(padded(stride, ofs)).cuda()
            got = _counts_of(m, lambda: m.observe_frames_dev(d.data_ptr() + ofs, N, w, h, stride, h * stride))
            _same(got, want, "device, offset %d stride %d" % (ofs, stride))
    # dword-aligned padded rows with a ragged end
    pad4 = (3 * w + 3) // 4 * 4 + 4
    d = torch.from_numpy(padded(pad4, 0)).cuda()
    _same(_counts_of(m, lambda: m.observe_frames_dev(d.data_ptr(), N, w, h, pad4, h * pad4)), want, "device, dword rows")
    # the sequence split over calls: the last frame of a call pairs with the first of the next; calls of one frame
    for split in ((23,), (1, 22), (5, 7, 11), (11, 1, 11)):
        edges = np.cumsum((0,) + split)
        got = _counts_of(m, lambda: [m.observe_frames(frames[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        _same(got, want, "split %s" % (split,))
    d = torch.from_numpy(frames).cuda()
    fb = w * h * 3
    got = _counts_of(m, lambda: [m.observe_frames_dev(d.data_ptr() + a * fb, b - a, w, h) for a, b in ((0, 5), (5, 12), (12, 23))])
    _same(got, want, "device split 5 + 7 + 11")
    m.activity_end()


# ---- 2. the observed image is the analysed image -----------------------------------------------------------------------------

def _by_taps(tap_images, delta=DELTA):
    return A.counts(np.stack(tap_images), delta)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_observed_yuv_frames_are_the_conversion_taps_images(capi, bare, fmt):
    import torch
    m, (w, h), n = bare, (640, 360), 7
    frames = A.moving_frames(n, h, w, 31)
    L, fb = capi.yuv420_layout(fmt, w, h)
    yuv = yref.frames_to_yuv(frames, L, fb)
    want = _by_taps([m.yuv420_to_bgr(y, w, h, L) for y in yuv])
    assert np.array_equal(m.yuv420_to_bgr(yuv[0], w, h, L), yref.to_bgr(yuv[0], w, h, L))
    assert want[0].any()
    _same(_counts_of(m, lambda: m.observe_frames_yuv420(yuv, w, h, L)), want, fmt + " host")
    d = torch.from_numpy(yuv).cuda()
    _same(_counts_of(m, lambda: [m.observe_frames_yuv420_dev(d.data_ptr(), 3, w, h, L, fb),
                                 m.observe_frames_yuv420_dev(d.data_ptr() + 3 * fb, n - 3, w, h, L, fb)]), want, fmt + " device, 3 + 4")
    m.activity_end()


def test_observed_p010_frames_under_a_description(capi):
    m, (w, h), n = capi.Matcher(small_cfg(capi)), (640, 360), 5
    desc = (dref.BT709, dref.LIMITED, dref.D10_MSB)
    m.set_yuv_description("bt709", "limited", "10_msb")
    frames = A.moving_frames(n, h, w, 32)
    L, fb = capi.yuv420_layout("nv12", w, h, bytes_per_sample=2)
    yuv = dref.frames_to_yuv(frames, L, fb, desc)
    taps = [m.yuv420_to_bgr(y, w, h, L) for y in yuv]
    assert np.array_equal(taps[0], dref.to_bgr(yuv[0], w, h, L, desc))
    want = _by_taps(taps)
    assert want[0].any()
    _same(_counts_of(m, lambda: m.observe_frames_yuv420(yuv, w, h, L)), want, "p010")
    # an 8-bit layout is refused under the 16-bit description, and the accumulator stays as it was
    L8, fb8 = capi.yuv420_layout("nv12", w, h)
    assert _code(capi, lambda: m.observe_frames_yuv420(np.zeros((1, fb8), np.uint8), w, h, L8))[0] == 1
    _same(m.activity_counts(), want, "after the refused layout")
    m.close()


def test_observed_frames_under_a_working_size(capi):
    m, n = capi.Matcher(small_cfg(capi)), 5
    m.set_working_size(640, 360)
    frames = A.moving_frames(n, 720, 1280, 33)
    want = _by_taps([m.reduce(f, 640, 360) for f in frames])
    assert want[0].shape == (360, 640) and want[0].any()
    _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "1280x720 under 640x360")
    m.close()


@pytest.mark.parametrize("quad,ow,oh", [([(20, 8), (419, 8), (419, 307), (20, 307)], 400, 300),
                                        ([(30.5, 20.25), (600.0, 12.5), (610.75, 338.0), (15.0, 330.5)], 402, 300)], ids=["crop", "keystone"])
def test_observed_frames_under_a_frame_region(capi, quad, ow, oh):
    import torch
    m, (w, h), n = capi.Matcher(small_cfg(capi)), (640, 360), 7
    m.set_frame_region(w, h, quad, ow, oh)
    frames = A.moving_frames(n, h, w, 34)
    want = _by_taps([m.rectify(f) for f in frames])
    assert want[0].shape == (oh, ow) and want[0].any()
    _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "region, host")
    d = torch.from_numpy(frames).cuda()
    _same(_counts_of(m, lambda: m.observe_frames_dev(d.data_ptr(), n, w, h)), want, "region, device")
    # the region's source-size rule, with the state unchanged
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :300]))
    assert c == 1 and "source size" in msg
    _same(m.activity_counts(), want, "after the refused size")
    m.close()


# ---- 3. the mask read-out ------------------------------------------------------------------------------------------------------

def _blinking_frames(w, h, n=9):
    """A still image in which regions toggle: on every frame (count = pairs), on every second pair and on every fourth — on all four
    borders, in a corner and inside."""
    rng = np.random.default_rng(w + h)
    base = rng.integers(0, 200, (h, w, 3), dtype=np.uint8)
    f = np.repeat(base[None], n, axis=0)

    def blink(ys, xs, period):
        for i in range(n):
            if (i // period) % 2:
                f[i, ys, xs] = base[ys, xs] + 40
    blink(slice(0, 2), slice(40, 90), 1)                  # top border, every pair
    blink(slice(h - 1, h), slice(100, 107), 1)            # bottom border
    blink(slice(50, 61), slice(0, 3), 2)                  # left border, every second pair
    blink(slice(70, 75), slice(w - 1, w), 1)              # right border
    blink(slice(h - 3, h), slice(w - 4, w), 2)            # a corner
    blink(slice(0, 1), slice(0, 1), 1)                    # the very corner pixel
    blink(slice(150, 153), slice(200, 209), 4)            # inside, every fourth pair
    blink(slice(h // 2, h // 2 + 1), slice(w // 2, w // 2 + 1), 2)
    return f


def test_mask_read_out_equals_the_restatement(capi, bare):
    m, (w, h) = bare, (349, 347)
    frames = _blinking_frames(w, h)
    count, pairs = A.counts(frames, DELTA)
    assert pairs == 8 and sorted(np.unique(count).tolist()) == [0, 2, 4, 8]
    _same(_counts_of(m, lambda: m.observe_frames(frames)), (count, pairs), "blinking")
    equal = 500000                                                 # count 4 of 8 pairs: 4e6 == 4e6, not active
    assert not A.active(count, pairs, equal)[count == 4].any() and A.active(count, pairs, equal - 1)[count == 4].all()
    seen = set()
    for ppm in (0, 1000000, equal, equal - 1, 250000):
        for grow in (0, 1, 7, 64):
            want, na, nm = A.mask(count, pairs, ppm, grow)
            got, gna, gnm = m.activity_mask(ppm / 1e6, grow)
            assert (gna, gnm) == (na, nm), (ppm, grow, gna, gnm, na, nm)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (ppm, grow, int((got != want).sum()))
            seen.add((na, nm))
    act, more = A.active(count, pairs, equal), A.active(count, pairs, equal - 1)
    assert act[0].any() and act[-1].any() and act[:, -1].any() and act[0, 0]          # top, bottom, right, the very corner
    assert more[50:61, 0].all() and not act[50:61, 0].any() and more[-1, -1]           # left border and a corner, at the equality
    assert (0, 0) in seen and len(seen) > 8                        # share 1000000: nothing is active
    m.activity_end()


# ---- 4. the rules ----------------------------------------------------------------------------------------------------------------

def test_rules_and_errors_leave_the_state_unchanged(capi, bare):
    import torch
    m, L, (w, h) = bare, capi.lib(), (402, 300)
    frames = A.moving_frames(6, h, w, 41)
    m.activity_end()
    m.activity_end()                                               # fine when the state is "none" already
    # without a begin
    assert _code(capi, lambda: m.observe_frames(frames))[0] == 4
    assert _code(capi, lambda: m.activity_info())[0] == 4
    assert _code(capi, lambda: m.activity_counts())[0] == 4
    assert _code(capi, lambda: m.activity_mask(0.5, 1))[0] == 4
    for bad in (-1, 766):
        assert _code(capi, lambda: m.activity_begin(bad))[0] == 1
    assert _code(capi, lambda: m.activity_info())[0] == 4          # the state before ("none") stays
    m.activity_begin(0); m.activity_begin(765)
    m.activity_begin(DELTA)
    assert m.activity_info() == {"aw": 0, "ah": 0, "pairs": 0, "delta": DELTA}
    assert _code(capi, lambda: m.activity_counts())[0] == 4        # no frame observed
    m.observe_frames(frames[:0].reshape(0, h, w, 3))               # n == 0: a no-op
    assert m.activity_info()["aw"] == 0
    m.observe_frames(frames[:1])
    assert m.activity_info() == {"aw": w, "ah": h, "pairs": 0, "delta": DELTA}
    assert _code(capi, lambda: m.activity_mask(0.5, 1))[0] == 4    # no pair yet
    assert not m.activity_counts()[0].any()
    m.observe_frames(frames[1:4])
    want = A.counts(frames[:4], DELTA)
    _same(m.activity_counts(), want, "1 + 3")

    def unchanged(what):
        _same(m.activity_counts(), want, what)
        assert m.activity_info() == {"aw": w, "ah": h, "pairs": 3, "delta": DELTA}, what
    for bad in (-1, 766):                                          # a refused begin leaves the accumulator as it was
        assert _code(capi, lambda: m.activity_begin(bad))[0] == 1
    unchanged("refused begin")
    # another analysed size: SLIDEO_ERR_STATE, naming both sizes
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :-2, :-6]))
    assert c == 4 and "%dx%d" % (w - 6, h - 2) in msg and "%dx%d" % (w, h) in msg
    unchanged("another size")
    # the argument rules of a frame source
    p = frames.ctypes.data
    fs = C.c_int64(w * h * 3)
    obs = L.slideo_matcher_observe_frames_bgr8
    assert obs(m._h, 2, None, w, h, w * 3, fs) == 1                                           # null frames
    assert obs(m._h, -1, p, w, h, w * 3, fs) == 1
    assert obs(m._h, 2, p, w, h, w * 3 - 1, fs) == 1                                          # image geometry
    assert obs(m._h, 2, p, 0, h, w * 3, fs) == 1
    assert obs(m._h, 2, p, w, h, w * 3, C.c_int64(w * h * 3 - 1)) == 1                        # frame stride
    assert "frame_stride" in L.slideo_last_error(m._h).decode()
    Ly, fby = capi.yuv420_layout("nv12", w, h)
    yuv = np.zeros((2, fby), np.uint8)
    assert L.slideo_matcher_observe_frames_yuv420(m._h, 2, yuv.ctypes.data, w, h, None, C.c_int64(fby)) == 1          # null layout
    assert L.slideo_matcher_observe_frames_yuv420(m._h, 2, yuv.ctypes.data, w + 1, h, C.byref(Ly), C.c_int64(fby)) == 5     # odd width
    bad = capi.Yuv420Layout.from_buffer_copy(Ly)
    bad.y_stride = w - 1
    assert L.slideo_matcher_observe_frames_yuv420(m._h, 2, yuv.ctypes.data, w, h, C.byref(bad), C.c_int64(fby)) == 1
    assert L.slideo_matcher_observe_frames_yuv420(m._h, 2, yuv.ctypes.data, w, h, C.byref(Ly), C.c_int64(fby - 1)) == 1     # frame stride
    unchanged("argument errors")
    # pairs would pass INT32_MAX: refused before a byte of the frames is read
    d = torch.from_numpy(frames).cuda()
    assert L.slideo_matcher_observe_frames_bgr8_dev(m._h, 2 ** 31 - 1, C.c_void_p(d.data_ptr()), w, h, w * 3, fs, None) == 4
    assert "INT32_MAX" in L.slideo_last_error(m._h).decode()
    unchanged("pairs past INT32_MAX")
    # the taps' own errors
    aw, ah, pr = C.c_int32(), C.c_int32(), C.c_int32()
    small = np.zeros(16, np.uint32)
    assert L.slideo_matcher_activity_counts(m._h, small.ctypes.data, C.c_int64(16), C.byref(aw), C.byref(ah), C.byref(pr)) == 7
    assert (aw.value, ah.value, pr.value) == (w, h, 3)
    aw, ah = C.c_int32(), C.c_int32()
    assert L.slideo_matcher_activity_counts(m._h, None, C.c_int64(0), C.byref(aw), C.byref(ah), C.byref(pr)) == 0 and (aw.value, ah.value) == (w, h)
    assert L.slideo_matcher_activity_counts(m._h, None, C.c_int64(0), None, C.byref(ah), C.byref(pr)) == 1
    na, nm = C.c_int64(), C.c_int64()
    out = np.zeros(w * h, np.uint8)
    mask = L.slideo_matcher_activity_mask
    aw, ah = C.c_int32(), C.c_int32()
    assert mask(m._h, 500000, 1, out.ctypes.data, C.c_int64(w * h - 1), C.byref(aw), C.byref(ah), C.byref(na), C.byref(nm)) == 7
    assert (aw.value, ah.value) == (w, h)
    for ppm, grow in ((-1, 1), (1000001, 1), (500000, -1), (500000, 65)):
        assert mask(m._h, ppm, grow, out.ctypes.data, C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(na), C.byref(nm)) == 1, (ppm, grow)
    assert mask(m._h, 500000, 1, None, C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(na), C.byref(nm)) == 1
    assert mask(m._h, 500000, 1, out.ctypes.data, C.c_int64(out.size), C.byref(aw), C.byref(ah), C.byref(na), None) == 1
    unchanged("tap errors")
    # a frame mask of another size, under the GATE scope too, does not refuse an observe; setters do not reset the accumulator
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(np.full((270, 480), 255, np.uint8))         # (at least small_area pixels, as every mask)
    m.set_direct_scope(capi.DIRECT_VALID)
    try:
        unchanged("setters")
        m.observe_frames(frames[4:])
        want = A.counts(frames, DELTA)
        _same(m.activity_counts(), want, "under a mask of another size")
        # a size that no longer fits is caught by the size rule
        m.set_working_size(200, 150)
        c, msg = _code(capi, lambda: m.observe_frames(frames[:1]))
        assert c == 4 and "%dx%d" % (w, h) in msg
        _same(m.activity_counts(), want, "a working size set in between")
    finally:
        m.set_working_size(0, 0)
        m.set_direct_scope(capi.DIRECT_WHOLE)
        m.set_frame_mask(None)
        m.set_frame_mask_scope(capi.MASK_DETECT)
    # begin resets; end, then observe
    m.activity_begin(3)
    assert m.activity_info() == {"aw": 0, "ah": 0, "pairs": 0, "delta": 3}
    m.observe_frames(frames[:2, :100, :200])                      # another size is fine after a begin
    _same(m.activity_counts(), A.counts(frames[:2, :100, :200], 3), "after begin")
    m.activity_end()
    assert _code(capi, lambda: m.observe_frames(frames))[0] == 4


def test_every_call_needs_an_idle_matcher(capi, cfg0_data):
    """While a submitted unit is uncollected, begin, end, the four observe calls and the two read-outs are SLIDEO_ERR_STATE; the
    unit's verdicts and the accumulator are what they are without those calls."""
    import torch
    pages, frames, _, _ = cfg0_data
    m, L, (w, h) = capi.Matcher(small_cfg(capi)), capi.lib(), (640, 360)
    m.add_pages(list(pages)); m.finalize()
    want_v = m.match_frames(frames)
    m.activity_begin(DELTA)
    m.observe_frames(frames[:5])
    want = A.counts(frames[:5], DELTA)
    _same(m.activity_counts(), want, "before the unit")
    Ly, fby = capi.yuv420_layout("nv12", w, h)
    yuv = yref.frames_to_yuv(frames[:2], Ly, fby)
    d, dy = torch.from_numpy(frames).cuda(), torch.from_numpy(yuv).cuda()
    tk = m.submit_dev(d.data_ptr(), 4, w, h)
    busy = {"begin": lambda: m.activity_begin(3), "end": m.activity_end,
            "observe host bgr": lambda: m.observe_frames(frames[5:]),
            "observe host yuv": lambda: m.observe_frames_yuv420(yuv, w, h, Ly),
            "observe device bgr": lambda: m.observe_frames_dev(d.data_ptr(), 2, w, h),
            "observe device yuv": lambda: m.observe_frames_yuv420_dev(dy.data_ptr(), 2, w, h, Ly, fby),
            "counts": m.activity_counts, "mask": lambda: m.activity_mask(0.5, 1)}
    for name, fn in busy.items():
        c, msg = _code(capi, fn)
        assert c == 4 and "collected" in msg, (name, c, msg)
    assert m.activity_info() == {"aw": w, "ah": h, "pairs": 4, "delta": DELTA}
    assert m.collect(tk).tobytes() == want_v[:4].tobytes()
    _same(m.activity_counts(), want, "after the refused calls")
    m.observe_frames(frames[5:])                                   # and the accumulator goes on where it was
    _same(m.activity_counts(), A.counts(frames, DELTA), "continued")
    m.close()


def test_sizes_are_refused_as_a_frame_call_refuses_them(capi, bare):
    """An analysed image, or the source of a frame the working size reduces, beyond 4096 a side: SLIDEO_ERR_UNSUPPORTED before a byte is
    read (device pointers of a small allocation), and the accumulator stays as it was."""
    import torch
    m, L = bare, capi.lib()
    frames = A.moving_frames(3, 33, 403, 44)
    want = A.counts(frames, DELTA)
    _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "before")
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(d.data_ptr())
    obs = L.slideo_matcher_observe_frames_bgr8_dev
    assert obs(m._h, 1, p, 4097, 2, 4097 * 3, C.c_int64(4097 * 6), None) == 5
    assert obs(m._h, 1, p, 2, 4097, 6, C.c_int64(4097 * 6), None) == 5
    m.set_working_size(640, 360)
    try:
        assert obs(m._h, 1, p, 4098, 2306, 4098 * 3, C.c_int64(4098 * 3 * 2306), None) == 5           # the source of a reduced frame
        assert "4098x2306" in L.slideo_last_error(m._h).decode()
    finally:
        m.set_working_size(0, 0)
    _same(m.activity_counts(), want, "after the refused sizes")
    m.activity_end()


def test_observing_touches_nothing_else(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    m = capi.Matcher(small_cfg(capi))
    m.activity_begin(DELTA)
    m.observe_frames(frames[:3])                                   # before any page is added and before finalize
    m.add_pages(list(pages)); m.finalize()
    other = A.moving_frames(5, 360, 640, 43)
    # verdicts of match_frames before and after an observation
    before = m.match_frames(frames)
    m.observe_frames(frames[3:])
    assert m.match_frames(frames).tobytes() == before.tobytes()
    _same(m.activity_counts(), A.counts(frames, DELTA), "around add_pages, finalize and match_frames")
    # the frames a mask call kept stay valid across an observe
    sel = np.arange(len(frames), dtype=np.int32)
    m.changed_mask(frames)
    want = m.match_kept_frames(sel)
    assert want.tobytes() == before.tobytes()
    m.changed_mask(frames)
    m.activity_begin(DELTA)
    m.observe_frames(other)
    got = m.match_kept_frames(sel)
    assert got.tobytes() == want.tobytes()
    # the gate state stays
    m.gate_reset(None)
    g1 = m.match_changed_frames(frames[:4])
    small = m.gate_last_small()
    m.observe_frames(other)
    assert np.array_equal(m.gate_last_small(), small)
    g2 = m.match_changed_frames(frames[3:])
    m.gate_reset(None)
    whole = m.match_changed_frames(np.concatenate([frames[:4], frames[3:]]))
    assert np.array_equal(np.concatenate([g1[0], g2[0]]), whole[0]) and np.concatenate([g1[2], g2[2]]).tobytes() == whole[2].tobytes()
    _same(m.activity_counts(), A.counts(np.concatenate([other, other]), DELTA), "beside gated calls")
    m.close()


# ---- 5. the use: a mask learnt from frames with a moving inset -----------------------------------------------------------------

W, H = 640, 360
HOLE = (190, 350, 390, 630)            # rows, columns of the hole in the hand-made 640x360 mask of tests/test_gpu_gate_mask.py
INSET = (191, 349, 391, 629)           # the inset: one pixel inside the hole on every side


def _rect_hole(h, w, y0, y1, x0, x1):
    m = np.full((h, w), 255, np.uint8)
    m[y0:y1, x0:x1] = 0
    return m


@pytest.fixture(scope="module")
def content(cfg0_data):
    """cfg0's 8 frames held [2, 3, 4, 2, 3, 4, 2, 3] times — 23 frames, 22 pairs — and the same with an inset re-randomised on every
    frame: the content of tests/test_gpu_gate_mask.py."""
    pages, frames, _, _ = cfg0_data
    reps = [2, 3, 4, 2, 3, 4, 2, 3]
    seq = np.ascontiguousarray(np.repeat(frames, reps, axis=0))
    held = np.ones(len(seq), bool)
    held[np.cumsum([0] + reps[:-1])] = False
    rng = np.random.default_rng(5)
    ins = seq.copy()
    y0, y1, x0, x1 = INSET
    for f in ins:
        f[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    return dict(pages=pages, seq=seq, ins=ins, held=held)


def test_learnt_mask_equals_the_hand_made_one_and_gates_like_it(capi, content):
    from slideo_amd import matching as mt
    c = content
    hole = _rect_hole(H, W, *HOLE)
    # on the restatement first
    count, pairs = A.counts(c["ins"], 24)
    assert pairs == 22
    y0, y1, x0, x1 = INSET
    inset = np.zeros((H, W), bool)
    inset[y0:y1, x0:x1] = True
    assert count[inset].min() >= 20 and count[~inset].max() <= 7
    ref_mask, na, nm = A.mask(count, pairs, 500000, 1)
    assert np.array_equal(ref_mask, hole) and na == int(inset.sum()) and nm == int((hole == 0).sum())
    # the library
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(c["pages"])); m.finalize()
    batches = [c["ins"][:9], c["ins"][9:10], c["ins"][10:]]
    learnt = mt.learn_frame_mask(m, batches, delta=24, max_share=0.5, grow=1)
    assert learnt.dtype == np.uint8 and learnt.tobytes() == hole.tobytes()
    assert _code(capi, lambda: m.activity_info())[0] == 4          # learn_frame_mask ended the accumulator
    # the same sequence without an inset: no pixel is active at 0.5
    m.activity_begin(24)
    m.observe_frames(c["seq"])
    clean, na0, nm0 = m.activity_mask(0.5, 1)
    m.activity_end()
    assert (na0, nm0) == (0, 0) and (clean == 255).all()
    # without a mask the inset defeats the gate on every frame; under the learnt mask exactly the frames that are not held are flagged
    m.gate_reset(None)
    assert m.match_changed_frames(c["ins"])[0].all()
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(learnt)
    m.gate_reset(None)
    changed = m.match_changed_frames(c["ins"])[0]
    assert np.array_equal(changed, ~c["held"]), changed
    m.close()
