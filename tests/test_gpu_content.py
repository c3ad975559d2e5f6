"""Frame content box (include/slideo_amd.h "Frame content box") on the GPU: the lit counts through the tap against ONE numpy
restatement (tests/content_ref.py) on every path frames arrive by, the observed image against the images the taps return, the
read-out (box, n_content, both fill arrays), both accumulators open in one pass, the rules, and the use the feature is for: the
region learnt from pillarboxed frames is the exact crop, and under it the direct page look-up resolves every changed frame."""
import ctypes as C

import numpy as np
import pytest

import activity_ref as A
import content_ref as R
import gate_mask_ref as gref
import yuv420_ref as yref
import yuv_desc_ref as dref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

LEVEL = R.LEVEL


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


def _counts_of(m, observe, level=LEVEL):
    m.content_begin(level)
    observe()
    return m.content_counts()


def _same(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), "%s: %d counts differ" % (what, int((got[0] != want[0]).sum()))


def _dev(frames, kind, ofs):
    """-> (tensor, pointer, stride, frame stride) of the frames on the device in the layout `kind` at a base offset of `ofs` bytes"""
    import torch
    n, h, w, _ = frames.shape
    stride = R.strides(w)[kind]
    d = torch.from_numpy(R.padded(frames, stride, ofs, fill=0xFF)).cuda()
    return d, d.data_ptr() + ofs, stride, h * stride


# ---- 1. counts equal the restatement, on every path --------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.COUNT_SIZES + [R.BIG[:2]], ids=lambda v: str(v))
def test_counts_equal_the_restatement(capi, bare, w, h):
    m, L = bare, capi.lib()
    for n in ((R.BIG[2],) if (w, h) == R.BIG[:2] else R.FRAME_COUNTS):
        frames = R.level_frames(n, h, w, w * 7 + h + n)
        want = R.counts(frames, LEVEL)
        assert want[1] == n and (w * h < 4 or 0 < int((want[0] > 0).sum()) < w * h)
        _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "host, %d frames" % n)
        assert m.content_info() == {"aw": w, "ah": h, "frames": n, "level": LEVEL}
        for kind, ofs in R.layouts(n):
            d, p, stride, fs = _dev(frames, kind, ofs)
            _same(_counts_of(m, lambda: m.observe_frames_dev(p, n, w, h, stride, fs)), want, "device, %d frames, %s + %d" % (n, kind, ofs))
        if n == 5:                                                 # host frames with a padded stride
            stride = R.strides(w)["odd"]
            buf = R.padded(frames, stride, 0)
            _same(_counts_of(m, lambda: m._check(L.slideo_matcher_observe_frames_bgr8(m._h, n, buf.ctypes.data, w, h, stride, C.c_int64(h * stride)))),
                  want, "host, padded stride")
    # level 0 and 254
    frames = R.level_frames(3, h, w, w + h)
    frames[0, 0, 0] = [255, 0, 1]
    for level in (0, 254):
        _same(_counts_of(m, lambda: m.observe_frames(frames), level), R.counts(frames, level), "level %d" % level)
    m.content_end()


@pytest.mark.parametrize("w,h", [(67, 9), (640, 360)], ids=lambda v: str(v))
def test_counts_across_calls_and_blocks(capi, bare, w, h):
    """The same frames in one call and split 1 + 3 + 5: identical counts and frames."""
    m, n = bare, sum(R.SPLIT)
    frames = R.level_frames(n, h, w, w * 7 + h + n)
    want = R.counts(frames, LEVEL)
    whole = _counts_of(m, lambda: m.observe_frames(frames))
    _same(whole, want, "one call")
    edges = np.cumsum((0,) + R.SPLIT)
    parts = _counts_of(m, lambda: [m.observe_frames(frames[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    _same(parts, want, "host 1 + 3 + 5")
    assert parts[1] == whole[1] and np.array_equal(parts[0], whole[0])
    for kind in ("tight", "odd"):
        d, p, stride, fs = _dev(frames, kind, 0)
        got = _counts_of(m, lambda: [m.observe_frames_dev(p + int(a) * fs, int(b - a), w, h, stride, fs) for a, b in zip(edges[:-1], edges[1:])])
        _same(got, want, "device 1 + 3 + 5, " + kind)
    m.content_end()


# ---- 2. the observed image is the analysed image -----------------------------------------------------------------------------

def _by_taps(tap_images, level=LEVEL):
    want = R.counts(np.stack(tap_images), level)
    assert want[0].any() and (want[0] < want[1]).any()
    return want


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_observed_yuv_frames_are_the_conversion_taps_images(capi, bare, fmt):
    import torch
    m, (w, h), n = bare, (640, 360), 5
    frames = R.level_frames(n, h, w, 31)
    L, fb = capi.yuv420_layout(fmt, w, h)
    yuv = yref.frames_to_yuv(frames, L, fb)
    want = _by_taps([m.yuv420_to_bgr(y, w, h, L) for y in yuv])
    assert np.array_equal(m.yuv420_to_bgr(yuv[0], w, h, L), yref.to_bgr(yuv[0], w, h, L))
    _same(_counts_of(m, lambda: m.observe_frames_yuv420(yuv, w, h, L)), want, fmt + " host")
    d = torch.from_numpy(yuv).cuda()
    _same(_counts_of(m, lambda: [m.observe_frames_yuv420_dev(d.data_ptr(), 2, w, h, L, fb),
                                 m.observe_frames_yuv420_dev(d.data_ptr() + 2 * fb, n - 2, w, h, L, fb)]), want, fmt + " device, 2 + 3")
    m.content_end()


def test_observed_p010_frames_under_a_description(capi):
    m, (w, h), n = capi.Matcher(small_cfg(capi)), (640, 360), 5
    desc = (dref.BT709, dref.LIMITED, dref.D10_MSB)
    m.set_yuv_description("bt709", "limited", "10_msb")
    frames = R.level_frames(n, h, w, 32)
    L, fb = capi.yuv420_layout("nv12", w, h, bytes_per_sample=2)
    yuv = dref.frames_to_yuv(frames, L, fb, desc)
    taps = [m.yuv420_to_bgr(y, w, h, L) for y in yuv]
    assert np.array_equal(taps[0], dref.to_bgr(yuv[0], w, h, L, desc))
    _same(_counts_of(m, lambda: m.observe_frames_yuv420(yuv, w, h, L)), _by_taps(taps), "p010")
    m.close()


def test_observed_frames_under_a_working_size(capi):
    """1280x720 frames under a 640x360 working size: the reduce is its 2x2 instance."""
    m, n = capi.Matcher(small_cfg(capi)), 5
    m.set_working_size(640, 360)
    frames = R.level_frames(n, 720, 1280, 33)
    want = _by_taps([m.reduce(f, 640, 360) for f in frames])
    assert want[0].shape == (360, 640)
    _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "1280x720 under 640x360")
    m.close()


def test_observed_frames_under_an_integer_crop_region(capi):
    import torch
    m, (w, h), n = capi.Matcher(small_cfg(capi)), (640, 360), 5
    m.set_frame_region(w, h, [(20, 8), (419, 8), (419, 307), (20, 307)], 400, 300)
    frames = R.level_frames(n, h, w, 34)
    taps = [m.rectify(f) for f in frames]
    assert np.array_equal(taps[0], frames[0, 8:308, 20:420])      # the integer translation: the crop itself
    want = _by_taps(taps)
    assert want[0].shape == (300, 400)
    _same(_counts_of(m, lambda: m.observe_frames(frames)), want, "region, host")
    d = torch.from_numpy(frames).cuda()
    _same(_counts_of(m, lambda: m.observe_frames_dev(d.data_ptr(), n, w, h)), want, "region, device")
    m.close()


# ---- 3. the read-out -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.READ_SIZES, ids=lambda v: str(v))
def test_read_out_equals_the_restatement(capi, bare, w, h):
    m = bare
    frames = R.read_frames(w, h)
    lit, n = R.counts(frames, LEVEL)
    assert (lit[h // 2] == 2).all() and n == 4                     # a share of 0.5 is met with equality in the content
    _same(_counts_of(m, lambda: m.observe_frames(frames)), (lit, n), "read-out frames")
    boxes = set()
    for share in R.SHARES:
        for fill in R.FILLS:
            want = R.box(lit, n, int(round(share * 1e6)), int(round(fill * 1e6)))
            box, nc, rf, cf = m.content_box(share, fill)
            assert box == want[0] and nc == want[1], (share, fill, box, nc, want[:2])
            assert rf.dtype == np.uint32 and np.array_equal(rf, want[2]) and np.array_equal(cf, want[3]), (share, fill)
            boxes.add(box)
    assert (0, 0, 0, 0) in boxes and (w * h == 1 or len(boxes) > 1)
    m.content_end()


def test_an_all_dark_stream_has_an_empty_box(capi, bare):
    m = bare
    frames = np.random.default_rng(3).integers(0, LEVEL + 1, (3, 9, 67, 3), dtype=np.uint8)
    got = _counts_of(m, lambda: m.observe_frames(frames))
    assert got[1] == 3 and not got[0].any()
    for share, fill in ((0.0, 0.0), (0.5, 0.25)):
        box, nc, rf, cf = m.content_box(share, fill)               # SLIDEO_OK
        assert box == (0, 0, 0, 0) and nc == 0 and not rf.any() and not cf.any()
    m.content_end()


# ---- 4. both accumulators ------------------------------------------------------------------------------------------------------

def test_both_accumulators_open(capi, bare):
    m, (w, h), delta = bare, (260, 17), 24
    frames = R.level_frames(9, h, w, 51)
    calls = [frames[:1], frames[1:4], frames[4:]]
    m.activity_end(); m.content_end()
    m.activity_begin(delta)
    for c in calls:
        m.observe_frames(c)
    act_only = m.activity_counts()
    m.activity_end()
    cnt_only = _counts_of(m, lambda: [m.observe_frames(c) for c in calls])
    assert m.content_info()["frames"] == 9
    m.content_end()
    _same(act_only, A.counts(frames, delta), "activity only")
    _same(cnt_only, R.counts(frames, LEVEL), "content only")
    # both, the content session opened one call later than the activity session
    m.activity_begin(delta)
    m.observe_frames(calls[0])
    m.content_begin(LEVEL)
    m.observe_frames(calls[1]); m.observe_frames(calls[2])
    _same(m.activity_counts(), act_only, "activity beside content")
    _same(m.content_counts(), R.counts(frames[1:], LEVEL), "content beside activity")
    # a frame of another size: SLIDEO_ERR_STATE, names the accumulator, leaves both unchanged
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :-2, :-6]))
    assert c == 4 and "activity accumulator" in msg and "%dx%d" % (w, h) in msg
    _same(m.activity_counts(), act_only, "activity after the refused size")
    _same(m.content_counts(), R.counts(frames[1:], LEVEL), "content after the refused size")
    assert m.activity_info()["pairs"] == 8 and m.content_info()["frames"] == 8
    # the sessions end independently: the activity session ends, the content session goes on, and the other way round
    m.activity_end()
    m.observe_frames(frames[:2])
    _same(m.content_counts(), R.counts(np.concatenate([frames[1:], frames[:2]]), LEVEL), "content after activity_end")
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :-2, :-6]))
    assert c == 4 and "content accumulator" in msg and "%dx%d" % (w, h) in msg
    m.activity_begin(delta)                                       # a fresh activity session takes another size only if content agrees
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :-2, :-6]))
    assert c == 4 and "content accumulator" in msg
    assert m.activity_info() == {"aw": 0, "ah": 0, "pairs": 0, "delta": delta}
    m.content_end()
    m.observe_frames(frames[:3, :-2, :-6])
    _same(m.activity_counts(), A.counts(frames[:3, :-2, :-6], delta), "activity after content_end")
    assert _code(capi, lambda: m.content_info())[0] == 4
    m.activity_end()


def test_activity_only_is_untouched(capi, bare):
    m, (w, h), delta = bare, (67, 9), 24
    frames = A.moving_frames(7, h, w, 52)
    m.content_end()
    m.activity_begin(delta)
    m.observe_frames(frames[:3]); m.observe_frames(frames[3:])
    assert _code(capi, lambda: m.content_info())[0] == 4
    assert _code(capi, lambda: m.content_counts())[0] == 4
    count, pairs = A.counts(frames, delta)
    _same(m.activity_counts(), (count, pairs), "activity only")
    want = A.mask(count, pairs, 300000, 1)
    got = m.activity_mask(0.3, 1)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    m.activity_end()
    c, msg = _code(capi, lambda: m.observe_frames(frames))
    assert c == 4 and "slideo_matcher_activity_begin first" in msg          # with neither open: the message of before


# ---- 5. the rules ----------------------------------------------------------------------------------------------------------------

def test_rules_and_errors_leave_the_state_unchanged(capi, bare):
    import torch
    m, L, (w, h) = bare, capi.lib(), (67, 9)
    frames = R.level_frames(6, h, w, 41)
    m.activity_end()
    m.content_end()
    m.content_end()                                                # fine when the state is "none" already
    # without a begin
    assert _code(capi, lambda: m.observe_frames(frames))[0] == 4
    assert _code(capi, lambda: m.content_info())[0] == 4
    assert _code(capi, lambda: m.content_counts())[0] == 4
    box, nc = (C.c_int32 * 4)(), C.c_int64()
    assert L.slideo_matcher_content_box(m._h, 500000, 250000, box, C.byref(nc), None, C.c_int64(0)) == 4
    for bad in (-1, 255):
        assert _code(capi, lambda: m.content_begin(bad))[0] == 1
    assert _code(capi, lambda: m.content_info())[0] == 4           # the state before ("none") stays
    m.content_begin(0); m.content_begin(254)
    m.content_begin(LEVEL)
    assert m.content_info() == {"aw": 0, "ah": 0, "frames": 0, "level": LEVEL}
    assert _code(capi, lambda: m.content_counts())[0] == 4         # counts and box before a frame
    assert L.slideo_matcher_content_box(m._h, 500000, 250000, box, C.byref(nc), None, C.c_int64(0)) == 4
    m.observe_frames(frames[:0].reshape(0, h, w, 3))               # n == 0: a no-op
    assert m.content_info()["aw"] == 0
    m.observe_frames(frames[:1]); m.observe_frames(frames[1:4])
    want = R.counts(frames[:4], LEVEL)

    def unchanged(what):
        _same(m.content_counts(), want, what)
        assert m.content_info() == {"aw": w, "ah": h, "frames": 4, "level": LEVEL}, what
    unchanged("1 + 3")
    for bad in (-1, 255):                                          # a refused begin leaves the accumulator as it was
        assert _code(capi, lambda: m.content_begin(bad))[0] == 1
    unchanged("refused begin")
    # ppm out of range, null pointers
    fill = np.zeros(w + h, np.uint32)
    cbox = L.slideo_matcher_content_box
    for share, fl in ((-1, 0), (1000001, 0), (0, -1), (0, 1000001)):
        assert cbox(m._h, share, fl, box, C.byref(nc), fill.ctypes.data, C.c_int64(fill.size)) == 1, (share, fl)
    assert cbox(m._h, 500000, 250000, None, C.byref(nc), None, C.c_int64(0)) == 1
    assert cbox(m._h, 500000, 250000, box, None, None, C.c_int64(0)) == 1
    # the capacity errors
    assert cbox(m._h, 500000, 250000, box, C.byref(nc), fill.ctypes.data, C.c_int64(w + h - 1)) == 7
    assert cbox(m._h, 500000, 250000, box, C.byref(nc), None, C.c_int64(0)) == 0          # fill_out is optional
    assert (tuple(box), nc.value) == R.box(want[0], 4, 500000, 250000)[:2]
    aw, ah, fr = C.c_int32(), C.c_int32(), C.c_int32()
    small = np.zeros(16, np.uint32)
    assert L.slideo_matcher_content_counts(m._h, small.ctypes.data, C.c_int64(16), C.byref(aw), C.byref(ah), C.byref(fr)) == 7
    assert (aw.value, ah.value, fr.value) == (w, h, 4)             # with the sizes set
    aw, ah = C.c_int32(), C.c_int32()
    assert L.slideo_matcher_content_counts(m._h, None, C.c_int64(0), C.byref(aw), C.byref(ah), C.byref(fr)) == 0 and (aw.value, ah.value) == (w, h)
    assert L.slideo_matcher_content_counts(m._h, None, C.c_int64(0), None, C.byref(ah), C.byref(fr)) == 1
    assert L.slideo_matcher_content_info(m._h, C.byref(aw), C.byref(ah), C.byref(fr), None) == 1
    unchanged("tap errors")
    # another analysed size, an argument error, frames past INT32_MAX (refused before a byte of the frames is read)
    c, msg = _code(capi, lambda: m.observe_frames(frames[:, :-2, :-6]))
    assert c == 4 and "content accumulator" in msg and "%dx%d" % (w - 6, h - 2) in msg and "%dx%d" % (w, h) in msg
    assert L.slideo_matcher_observe_frames_bgr8(m._h, 2, None, w, h, w * 3, C.c_int64(w * h * 3)) == 1
    d = torch.from_numpy(frames).cuda()
    assert L.slideo_matcher_observe_frames_bgr8_dev(m._h, 2 ** 31 - 4, C.c_void_p(d.data_ptr()), w, h, w * 3, C.c_int64(w * h * 3), None) == 4
    assert "INT32_MAX" in L.slideo_last_error(m._h).decode() and "content" in L.slideo_last_error(m._h).decode()
    unchanged("refused observes")
    # begin resets; end, then observe
    m.content_begin(3)
    assert m.content_info() == {"aw": 0, "ah": 0, "frames": 0, "level": 3}
    m.observe_frames(frames[:2, :5, :30])                         # another size is fine after a begin
    _same(m.content_counts(), R.counts(frames[:2, :5, :30], 3), "after begin")
    m.content_end()
    assert _code(capi, lambda: m.observe_frames(frames))[0] == 4


def test_every_call_needs_an_idle_matcher(capi, cfg0_data):
    """While a submitted unit is uncollected, begin, end, counts and box are SLIDEO_ERR_STATE; the unit's verdicts and the
    accumulator are what they are without those calls."""
    import torch
    pages, frames, _, _ = cfg0_data
    m, (w, h) = capi.Matcher(small_cfg(capi)), (640, 360)
    m.add_pages(list(pages)); m.finalize()
    want_v = m.match_frames(frames)
    m.content_begin(LEVEL)
    m.observe_frames(frames[:5])
    want = R.counts(frames[:5], LEVEL)
    _same(m.content_counts(), want, "before the unit")
    d = torch.from_numpy(frames).cuda()
    tk = m.submit_dev(d.data_ptr(), 4, w, h)
    busy = {"begin": lambda: m.content_begin(3), "end": m.content_end, "observe": lambda: m.observe_frames(frames[5:]),
            "counts": m.content_counts, "box": lambda: m.content_box(0.5, 0.25)}
    for name, fn in busy.items():
        c, msg = _code(capi, fn)
        assert c == 4 and "collected" in msg, (name, c, msg)
    assert m.content_info() == {"aw": w, "ah": h, "frames": 5, "level": LEVEL}
    assert m.collect(tk).tobytes() == want_v[:4].tobytes()
    _same(m.content_counts(), want, "after the refused calls")
    m.observe_frames(frames[5:])                                   # and the accumulator goes on where it was
    _same(m.content_counts(), R.counts(frames, LEVEL), "continued")
    assert m.match_frames(frames).tobytes() == want_v.tobytes()    # observing touches nothing else
    m.close()


# ---- 6. the use: 4:3 pages pillarboxed in 16:9 frames ----------------------------------------------------------------------------

SHOWN = [0, 0, 1, 2, 2, 3, 4, 5, 5, 0, 1, 1]


def test_learnt_region_is_the_exact_crop_and_the_direct_look_up_applies(capi, synth):
    from slideo_amd import matching as mt
    pages = synth.pages(6, 480, 360)
    rng = np.random.default_rng(18)
    frames = rng.integers(0, LEVEL + 1, (len(SHOWN), 360, 640, 3), dtype=np.uint8)      # the bars: noise in 0..level
    for i, p in enumerate(SHOWN):
        frames[i, :, 80:560] = pages[p]                            # the content: the page itself, no noise
    # the precondition, on the restatement: under these thresholds the box of these frames is the pasted page's, and every row and
    # column of every page is content on its own
    lit, n = R.counts(frames, LEVEL)
    assert R.box(lit, n, 500000, 250000)[0] == (80, 0, 560, 360)
    for p in range(6):
        pl, _ = R.counts(pages[p:p + 1], LEVEL)
        assert R.box(pl, 1, 500000, 250000)[0] == (0, 0, 480, 360)
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    region = mt.learn_frame_region(m, [frames[:5], frames[5:6], frames[6:]], level=LEVEL, min_share=0.5, min_fill=0.25)
    assert region == (640, 360, [(80.0, 0.0), (559.0, 0.0), (559.0, 359.0), (80.0, 359.0)], 480, 360)
    assert _code(capi, lambda: m.content_info())[0] == 4          # learn_frame_region ended the accumulator
    m.set_direct_similarity(0.99)
    # without a region: no page has the frame's small size, no direct verdict
    m.gate_reset(None)
    ch0, _, v0 = m.match_changed_frames(frames)
    assert ch0[0] and not ((v0["page_idx"] >= 0) & (v0["inliers"] == 0)).any()
    # with it: every changed frame is resolved directly, for the page it shows, at the identity's similarity
    m.set_frame_region(*region)
    assert np.array_equal(m.rectify(frames[3]), pages[SHOWN[3]])  # the rectified image is the page byte for byte
    m.gate_reset(None)
    ch, sim, v = m.match_changed_frames(frames)
    held = np.array([i > 0 and SHOWN[i] == SHOWN[i - 1] for i in range(len(SHOWN))])
    assert ch[0] and ch.sum() >= 2 and not ch[held].any(), ch     # the bars' noise is cropped: a held frame is byte-identical
    sh, sw, _ = m.page_small(0).shape
    for i in np.nonzero(ch)[0]:
        assert (v[i]["page_idx"], v[i]["inliers"], v[i]["n_keypoints"]) == (SHOWN[i], 0, 0), (i, v[i])
        assert v[i]["similarity"] == gref.similarity(0, sw * sh), (i, v[i])
    # the frame region's own contract: the same call on the cropped frames with no region
    m2 = capi.Matcher(small_cfg(capi))
    m2.add_pages(list(pages)); m2.finalize()
    m2.set_direct_similarity(0.99)
    m2.gate_reset(None)
    ch2, sim2, v2 = m2.match_changed_frames(np.ascontiguousarray(frames[:, :, 80:560]))
    assert np.array_equal(ch, ch2) and np.array_equal(sim.view(np.uint32), sim2.view(np.uint32)) and v.tobytes() == v2.tobytes()
    m.close(); m2.close()
