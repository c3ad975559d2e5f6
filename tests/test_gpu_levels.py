"""Frame levels (include/slideo_amd.h "Frame levels") on the GPU: the tap is bit-exact against the numpy restatement
(tests/levels_ref.py) over sizes and strides that make both loads and both stores of levels_kernel run; every call form that stages
frames returns under a table exactly what the same form returns under the default on the restatement's levelled images — both
doors, another pixel format, a working size, a frame region, SIFT mode, a group —; device frames are never written; the kept frames
of a mask call are not levelled twice; the refusals and the state each leaves; and the use case: a dim recording, the table learnt on
the GPU.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import levels_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _same3(a, b):
    """(changed, similarity, verdicts) of two gated calls."""
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


LUT = R.random_lut(11)


# ---- 1. the tap, bit-exact ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


@pytest.mark.parametrize("table", ["random", "stretch", "identity"])
def test_tap_bit_exact(capi, tap, table):
    lut = {"random": LUT, "stretch": R.stretch_lut([34, 20, 0], [106, 255, 90]), "identity": R.identity()}[table]
    tap.set_frame_levels(lut)
    if table == "identity":
        assert tap.frame_levels() is None                         # stored as off
    else:
        assert np.array_equal(tap.frame_levels(), lut)
    rng = np.random.default_rng(len(table))
    for w, h in R.SIZES:
        for stride in R.strides(w):
            buf = rng.integers(0, 256, h * stride, dtype=np.uint8)
            img = np.ascontiguousarray(buf.reshape(h, stride)[:, :3 * w]).reshape(h, w, 3)
            got = tap.levels_bgr((buf, w, h), stride=stride)
            assert np.array_equal(got, R.apply(img, lut)), (table, w, h, stride, np.argwhere(got != R.apply(img, lut))[:4])
    img = rng.integers(0, 256, (33, 130, 3), dtype=np.uint8)
    assert np.array_equal(tap.levels_bgr(img), R.apply(img, lut))
    tap.set_frame_levels(None)
    assert tap.frame_levels() is None and np.array_equal(tap.levels_bgr(img), img)
    L, out, on = capi.lib(), np.empty((3, 256), np.uint8), C.c_int32(7)
    assert L.slideo_matcher_frame_levels(tap._h, out.ctypes.data_as(C.c_void_p), C.byref(on)) == 0 and on.value == 0
    assert np.array_equal(out, R.identity())


# ---- 2. every call form under a table equals its default twin on the levelled images ---------------------------------------------------

@pytest.fixture(scope="module")
def deck(cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.ascontiguousarray(np.repeat(frames, 2, axis=0))      # every frame twice: changed and unchanged flags both occur
    # the random table scrambles the picture; a mild monotonic one keeps it matchable, so that verdicts of every kind occur
    return pages, seq


MILD = np.stack([np.clip(np.arange(256) * g + o, 0, 255).astype(np.uint8) for g, o in ((0.8, 20), (1.1, -10), (0.9, 5))])


def _matcher(capi, pages, lut=None, sift=None):
    m = capi.Matcher(small_cfg(capi))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if lut is not None:
        m.set_frame_levels(lut)
    return m


@pytest.fixture(scope="module", params=["mild", "random"])
def pair(request, capi, deck):
    """A matcher under the table, a matcher under the default, the sequence and the restatement's levelled images of it."""
    lut = MILD if request.param == "mild" else LUT
    pages, seq = deck
    n, h, w, _ = seq.shape
    m, ref = _matcher(capi, pages, lut), _matcher(capi, pages)
    yield request.param, lut, m, ref, seq, R.apply(seq, lut), w, h
    m.close(); ref.close()


def _device_frames(frames, ofs, pitch_extra=0, slack=0):
    """The frames in device memory, rows pitch_extra bytes beyond tight, frames `slack` bytes beyond a frame apart, the first byte
    `ofs` bytes past the allocation's base -> (tensor kept alive, pointer, stride, frame stride, the bytes as uploaded)."""
    import torch
    n, h, w, _ = frames.shape
    stride = 3 * w + pitch_extra
    fs = h * stride + slack
    host = np.random.default_rng(ofs + pitch_extra).integers(0, 256, n * fs, dtype=np.uint8)
    for i in range(n):
        host[i * fs: i * fs + h * stride].reshape(h, stride)[:, :3 * w] = frames[i].reshape(h, 3 * w)
    t = torch.empty(ofs + host.size, dtype=torch.uint8, device="cuda")
    t[ofs:].copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    return t, t.data_ptr() + ofs, stride, fs, host


def _untouched(t, ofs, host):
    return np.array_equal(t[ofs:].cpu().numpy(), host)


def test_match_frames_host_device_and_streaming(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    n = len(seq)
    want = ref.match_frames(lev)
    c_want = [ref.last_candidates(i) for i in range(n)]
    if name == "mild":
        assert (want["page_idx"] >= 0).mean() >= 0.5
    assert _same(m.match_frames(seq), want)
    for i in range(n):
        assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    for ofs, extra, slack in ((0, 0, 0), (1, 0, 0), (2, 1, 3), (4, 8, 12)):
        t, p, stride, fs, host = _device_frames(seq, ofs, extra, slack)
        assert _same(m.match_frames_dev(p, n, w, h, stride, fs), want), (ofs, extra, slack)
        for i in range(n):
            assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d from a device base offset of %d" % (i, ofs)
        assert _untouched(t, ofs, host), "the caller's device frames were written (base offset %d)" % ofs
    t, p, stride, fs, host = _device_frames(seq, 0)
    got, pend = [], []
    for i in range(0, n, 4):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_dev(p + i * fs, min(4, n - i), w, h))
    c, _ = _code(capi, lambda: m.set_frame_levels(None))          # a busy matcher refuses the setter, and the table stays
    assert c == 4 and np.array_equal(m.frame_levels(), lut)
    got += [m.collect(t_) for t_ in pend]
    assert _same(np.concatenate(got), want)
    assert _untouched(t, 0, host)


def test_changed_mask_and_kept_frames_are_not_levelled_twice(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    ch, sim, last = ref.changed_mask(lev)
    assert ch.any() and not ch.all()
    kept_want = ref.match_kept_frames([0, 3, 4])
    gc, gs, gl = m.changed_mask(seq)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    # (a second level of the table would be another picture: the twin on twice-levelled frames differs wherever one matched)
    if name == "mild":
        twice = ref.match_frames(R.apply(lev, lut)[[0, 3, 4]])
        assert not _same(twice, kept_want)
    gc2, gs2, gl2 = m.changed_mask(seq[3:], prev_small=gl)
    ch2, sim2, last2 = ref.changed_mask(lev[3:], prev_small=last)
    assert np.array_equal(gc2, ch2) and _same(gs2, sim2) and np.array_equal(gl2, last2)


@pytest.mark.parametrize("gate", ["previous", "anchor_settle", "anchor_memory"])
def test_gated_calls(capi, pair, gate):
    name, lut, m, ref, seq, lev, w, h = pair
    n = len(seq)
    for x in (m, ref):
        if gate != "previous":
            x.set_gate_reference("anchor")
        if gate == "anchor_settle":
            x.set_gate_settle(0.99, 2)
        if gate == "anchor_memory":
            x.set_gate_memory(4)
        x.gate_reset()
    try:
        want = [ref.match_changed_frames(lev[:5]), ref.match_changed_frames(lev[5:])]
        want_small = ref.gate_last_small()
        got = [m.match_changed_frames(seq[:5]), m.match_changed_frames(seq[5:])]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1])
        assert np.array_equal(m.gate_last_small(), want_small)
        if gate == "anchor_memory":                               # (the refs exist under a gate memory; the state record does not)
            assert np.array_equal(m.last_gate_refs(), ref.last_gate_refs())
            t, p, stride, fs, host = _device_frames(seq, 2, 0, 0)
            m.gate_reset(); ref.gate_reset()
            assert _same3(m.match_changed_frames_dev(p, n, w, h, stride, fs), ref.match_changed_frames(lev))
            assert np.array_equal(m.last_gate_refs(), ref.last_gate_refs()) and _untouched(t, 2, host)
            return
        assert m.gate_state_export() == ref.gate_state_export()
        t, p, stride, fs, host = _device_frames(seq, 1, 4, 8)
        m.gate_reset()
        got = [m.match_changed_frames_dev(p, 5, w, h, stride, fs), m.match_changed_frames_dev(p + 5 * fs, n - 5, w, h, stride, fs)]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1]) and m.gate_state_export() == ref.gate_state_export()
        m.gate_reset()
        tickets = [m.submit_changed_dev(p, 5, w, h, stride, fs), m.submit_changed_dev(p + 5 * fs, n - 5, w, h, stride, fs)]
        for tk, wnt in zip(tickets, want):
            assert _same3(m.collect_changed(tk), wnt)
        assert m.gate_state_export() == ref.gate_state_export()
        ref.gate_reset_from_frame(lev[2])
        a = ref.match_changed_frames(lev[3:6])
        m.gate_reset_from_frame(seq[2])
        assert m.gate_state_export() != b"" and _same3(m.match_changed_frames(seq[3:6]), a)
        assert np.array_equal(m.gate_last_small(), ref.gate_last_small())
        m.gate_reset_from_frame_dev(p + 2 * fs, w, h, stride)
        assert _same3(m.match_changed_frames_dev(p + 3 * fs, 3, w, h, stride, fs), a)
        assert m.gate_state_export() == ref.gate_state_export()
        # slideo_matcher_gate_reset(small) is untouched: the small image is taken as it is
        small = ref.gate_last_small()
        for x in (m, ref):
            x.gate_reset(small)
        assert m.gate_state_export() == ref.gate_state_export()
        assert _untouched(t, 1, host)
    finally:
        for x in (m, ref):
            x.set_gate_memory(0)
            x.set_gate_settle(0, 0)
            x.set_gate_reference("previous")
            x.gate_reset()


def test_observe_frames_activity_and_content(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    for x, f in ((ref, lev), (m, seq)):
        x.activity_begin(12)
        x.content_begin(24)
        x.observe_frames(f[:2])
        x.observe_frames(f[2:7])
    t, p, stride, fs, host = _device_frames(seq, 2, 0, 3)
    m.observe_frames_dev(p + 7 * fs, 3, w, h, stride, fs)
    ref.observe_frames(lev[7:10])
    a, b = m.activity_counts(), ref.activity_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 9 and b[0].any()
    a, b = m.content_counts(), ref.content_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 10
    assert _untouched(t, 2, host)
    for x in (m, ref):
        x.activity_end()
        x.content_end()


def test_frame_features_tap(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    sel = [1, 2, 6]
    feats = [ref.orb(lev[i]) for i in sel]                        # (the single-image tap is untouched: the levelled image's features)
    kps, descs = [f[0] for f in feats], [f[1] for f in feats]
    want = ref.match_features(lev[sel], kps, descs)
    assert _same(m.match_features(seq[sel], kps, descs), want)
    for i in range(len(sel)):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    assert np.array_equal(m.orb(seq[1])[1], ref.orb(seq[1])[1])   # pages and single-image taps do not see the table


def test_under_a_working_size_a_region_and_another_pixel_format(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    t, p, stride, fs, host = _device_frames(seq, 0, 4, 0)
    # a working size: the levels of the reduce tap's image
    m.set_working_size(480, 270)
    try:
        red = np.stack([ref.reduce(seq[i], 480, 270) for i in range(0, 12, 2)])
        want = ref.match_frames(R.apply(red, lut))
        assert _same(m.match_frames(seq[0:12:2]), want)
        red6 = np.stack([ref.reduce(seq[i], 480, 270) for i in range(6)])
        assert _same(m.match_frames_dev(p, 6, w, h, stride, fs), ref.match_frames(R.apply(red6, lut)))
        ch, sim, last = ref.changed_mask(R.apply(red6, lut))
        gc, gs, gl = m.changed_mask(seq[:6])
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        m.set_working_size(0, 0)
    # a frame region: the levels of the rectify tap's image
    quad = [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)]
    m.set_frame_region(w, h, quad, 480, 270)
    ref.set_frame_region(w, h, quad, 480, 270)
    try:
        rect = np.stack([ref.rectify(seq[i]) for i in range(6)])
        ref.clear_frame_region()
        lrect = R.apply(rect, lut)
        assert _same(m.match_frames(seq[:6]), ref.match_frames(lrect))
        for x in (m, ref):
            x.gate_reset()
        a = ref.match_changed_frames(lrect)
        assert _same3(m.match_changed_frames(seq[:6]), a)
        m.gate_reset()
        assert _same3(m.match_changed_frames_dev(p, 6, w, h, stride, fs), a)
    finally:
        for x in (m, ref):
            x.clear_frame_region()
            x.gate_reset()
    assert _untouched(t, 0, host)
    # another pixel format: the levels come behind the conversion
    m.set_pixel_format("rgba")
    try:
        rgba = np.concatenate([seq[:6, :, :, ::-1], np.full((6, h, w, 1), 99, np.uint8)], axis=3)
        assert np.array_equal(m.pixels_to_bgr(rgba[0]), seq[0])   # the conversion tap shows the image in front of the levels
        assert _same(m.match_frames(rgba), ref.match_frames(lev[:6]))
    finally:
        m.set_pixel_format("bgr")


def test_the_yuv_door(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = np.random.default_rng(1).integers(16, 236, (4, fb), dtype=np.uint8)
    yuv[2] = yuv[1]
    imgs = np.stack([ref.yuv420_to_bgr(yuv[i], w, h, L) for i in range(4)])
    assert np.array_equal(m.yuv420_to_bgr(yuv[0], w, h, L), imgs[0])      # the conversion tap: in front of the levels
    limgs = R.apply(imgs, lut)
    assert _same(m.match_frames_yuv420(yuv, w, h, L), ref.match_frames(limgs))
    for x in (m, ref):
        x.gate_reset()
    got, want = m.match_changed_frames_yuv420(yuv, w, h, L), ref.match_changed_frames(limgs)
    assert _same3(got, want) and np.array_equal(m.gate_last_small(), ref.gate_last_small())
    for x, f in ((m, None), (ref, limgs)):
        x.content_begin(40)
        if f is None:
            x.observe_frames_yuv420(yuv, w, h, L)
        else:
            x.observe_frames(f)
    assert np.array_equal(m.content_counts()[0], ref.content_counts()[0])
    for x in (m, ref):
        x.content_end()
        x.gate_reset()


def test_sift_mode(capi, deck):
    pages, seq = deck
    sift = (capi.sift_config(nfeatures=300), 0.0)
    m, ref = _matcher(capi, pages, MILD, sift), _matcher(capi, pages, None, sift)
    sel = seq[::3]
    want = ref.match_frames(R.apply(sel, MILD))
    assert (want["page_idx"] >= 0).any()
    assert _same(m.match_frames(sel), want)
    for i in range(len(sel)):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    m.close(); ref.close()


def test_group_of_two_members(capi, pair, deck):
    name, lut, m, ref, seq, lev, w, h = pair
    want = ref.match_frames(lev)
    ch, sim, last = ref.changed_mask(lev)
    kept = ref.match_kept_frames([1, 2, 9])
    ref.gate_reset()
    gated = ref.match_changed_frames(lev)
    ref.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    g.set_frame_levels(lut)
    assert np.array_equal(g.frame_levels(), lut)
    assert _same(g.match_frames(seq), want)
    gc, gs, gl = g.changed_mask(seq)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(g.match_kept_frames([1, 2, 9]), kept)
    assert _same3(g.match_changed_frames(seq), gated)
    # the group's setter validates every member before it changes any: member 1's open histogram refuses for both
    m1 = C.c_void_p(capi.lib().slideo_group_member(g._h, 1))
    g.set_frame_levels(None)
    assert capi.lib().slideo_matcher_levels_begin(m1) == 0
    c, msg = _code(capi, lambda: g.set_frame_levels(lut))
    assert c == 4 and "levels histogram" in msg and g.frame_levels() is None
    assert capi.lib().slideo_matcher_levels_end(m1) == 0
    g.set_frame_levels(lut)
    on = C.c_int32()
    assert capi.lib().slideo_matcher_frame_levels(m1, None, C.byref(on)) == 0 and on.value == 1
    g.close()


# ---- 3. refusals and the state each leaves ------------------------------------------------------------------------------------------

def test_refusals(capi, pair):
    name, lut, m, ref, seq, lev, w, h = pair
    # a session refuses while a table is set; the table stays and no session is open
    c, msg = _code(capi, m.levels_begin)
    assert c == 4 and "table" in msg and np.array_equal(m.frame_levels(), lut)
    assert _code(capi, m.levels_info)[0] == 4
    # setting a table refuses while the session is open; the session stays as it is
    m.set_frame_levels(None)
    m.levels_begin()
    m.observe_frames(seq[:2])
    c, msg = _code(capi, lambda: m.set_frame_levels(lut))
    assert c == 4 and "levels histogram" in msg and m.frame_levels() is None
    assert m.levels_info() == {"frames": 2, "pixels": 2 * w * h}
    # ... even off: the rule is the session's
    assert _code(capi, lambda: m.set_frame_levels(None))[0] == 4
    m.levels_end()
    # no frames observed: STATE for the read-outs, and the info of an empty session
    m.levels_begin()
    assert m.levels_info() == {"frames": 0, "pixels": 0}
    assert _code(capi, m.levels_histogram)[0] == 4 and _code(capi, lambda: m.levels_points(0.01, 0.01))[0] == 4
    m.levels_end()
    assert _code(capi, m.levels_info)[0] == 4
    # without any session the observe calls refuse
    assert _code(capi, lambda: m.observe_frames(seq[:1]))[0] == 4
    m.set_frame_levels(lut)
    # setting ends the kept frames and resets the gate state to "none"
    m.changed_mask(seq[:4])
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames(seq[:2])
    assert m.gate_last_small().ndim == 3
    m.changed_mask(seq[:4])
    m.set_frame_levels(lut)                                       # (the same table: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames(seq[1:3])
    assert ch[0]
    m.gate_reset()
    # the tap's capacity
    out = np.empty(10, np.uint8)
    img = np.zeros((4, 4, 3), np.uint8)
    assert capi.lib().slideo_levels_bgr8(m._h, img.ctypes.data_as(C.c_void_p), 4, 4, 12, out.ctypes.data_as(C.c_void_p), C.c_int64(10)) == 7


# ---- 4. the use case ---------------------------------------------------------------------------------------------------------------

def test_a_dim_recording_with_levels_learnt_on_the_gpu(capi, cfg0_data):
    from slideo_amd import matching as mt
    pages, frames, truth, _ = cfg0_data
    dark = R.darken(frames)
    m, ref = _matcher(capi, pages), _matcher(capi, pages)
    assert m.match_frames(dark)["page_idx"].tolist() == [-1] * 8
    m.levels_begin()
    m.observe_frames(dark[:3])
    m.observe_frames(dark[3:])
    assert m.levels_points(0.01, 0.01) == ([34] * 3, [106] * 3)
    assert np.array_equal(m.levels_histogram(), R.histogram(dark))
    m.levels_end()
    lut = mt.learn_frame_levels(m, [dark[:5], dark[5:]])
    assert np.array_equal(lut, R.stretch_lut([34] * 3, [106] * 3))
    assert m.frame_levels() is None                               # nothing is installed
    m.set_frame_levels(lut)
    with pytest.raises(ValueError):
        mt.learn_frame_levels(m, [dark])
    want = ref.match_frames(R.apply(dark, lut))
    got = m.match_frames(dark)
    assert _same(got, want) and got["page_idx"].tolist() == [int(t) for t in truth]
    for i in range(8):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    m.close(); ref.close()
