"""Frame shading (include/slideo_amd.h "Frame shading") on the GPU: the tap is bit-exact against the numpy restatement
(tests/shading_ref.py) over sizes, strides and cells that make both loads and both stores of shading_kernel run, with and without a
levels table (the fused instance equals shading then levels_ref.apply); every call form that stages frames returns under a field
exactly what the same form returns under the default on the restatement's shaded images — both doors, another pixel format, a
working size, a frame region, SIFT mode, a group —; device frames are never written; the kept frames of a mask call are not shaded
twice; a call at another analysed size fails; the refusals and the state each leaves.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import levels_ref as LR
import shading_ref as R
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


LUT = LR.random_lut(11)
MILD_LUT = np.stack([np.clip(np.arange(256) * g + o, 0, 255).astype(np.uint8) for g, o in ((0.8, 20), (1.1, -10), (0.9, 5))])


def _vignette(aw, ah, cell):
    """A mild, smooth field: 0.75 in the centre to 1.6 in the corners."""
    gw, gh = R.grid(aw, ah, cell)
    j, i = np.mgrid[0:gh + 1, 0:gw + 1].astype(np.float64)
    r2 = ((i * cell - aw / 2) / (aw / 2)) ** 2 + ((j * cell - ah / 2) / (ah / 2)) ** 2
    return np.rint(256 * (0.75 + 0.425 * r2)).astype(np.uint16)


# ---- 1. the tap, bit-exact ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("kind", ["random", "ramp", "identity"])
def test_tap_bit_exact(capi, tap, kind, table):
    rng = np.random.default_rng(len(kind) + table)
    tap.set_frame_levels(LUT if table else None)
    for w, h in R.SIZES:
        for cell in R.CELLS:
            g = {"random": R.random_field(w, h, cell, w + cell), "ramp": R.ramp_field(w, h, cell), "identity": R.identity(w, h, cell)}[kind]
            tap.set_frame_shading(w, h, cell, g)
            if kind == "identity":
                assert tap.frame_shading() is None                    # stored as off
            else:
                aw, ah, c, got = tap.frame_shading()
                assert (aw, ah, c) == (w, h, cell) and np.array_equal(got, g)
            for stride in R.strides(w):
                buf = rng.integers(0, 256, h * stride, dtype=np.uint8)
                img = np.ascontiguousarray(buf.reshape(h, stride)[:, :3 * w]).reshape(h, w, 3)
                want = R.apply(img, cell, g)
                if table and kind != "identity":                      # (no field: the tap is a copy, whatever the table)
                    want = LR.apply(want, LUT)
                got = tap.shading_bgr((buf, w, h), stride=stride)
                assert np.array_equal(got, want), (kind, table, w, h, cell, stride, np.argwhere(got != want)[:4])
    tap.set_frame_shading(gains=None)
    tap.set_frame_levels(None)
    img = rng.integers(0, 256, (33, 65, 3), dtype=np.uint8)
    assert tap.frame_shading() is None and np.array_equal(tap.shading_bgr(img), img)


def test_tap_refusals_and_the_getter(capi, tap):
    L = capi.lib()
    g = R.ramp_field(65, 33, 16)
    tap.set_frame_shading(65, 33, 16, g)
    img = np.zeros((33, 64, 3), np.uint8)
    c, msg = _code(capi, lambda: tap.shading_bgr(img))
    assert c == 1 and "65x33" in msg                              # another size than the field's
    out = np.empty(10, np.uint8)
    img = np.zeros((33, 65, 3), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.slideo_shading_bgr8(tap._h, p(img), 65, 33, 195, p(out), C.c_int64(10)) == 7
    v = [C.c_int32(-1) for _ in range(4)]
    few = np.full(4, 9, np.uint16)
    assert L.slideo_matcher_frame_shading(tap._h, p(few), C.c_int64(4), *[C.byref(x) for x in v]) == 7      # CAPACITY, the sizes set
    assert [x.value for x in v] == [65, 33, 16, 1] and (few == 9).all()
    assert L.slideo_matcher_frame_shading(tap._h, None, C.c_int64(0), *[C.byref(x) for x in v]) == 0         # the size query
    # a gain of 0, a bad cell, a bad size: refused, and the field before stays
    bad = g.copy(); bad[2, 3] = 0
    assert L.slideo_matcher_set_frame_shading(tap._h, 65, 33, 16, p(bad)) == 1
    assert "node (3, 2)" in L.slideo_last_error(tap._h).decode()
    assert L.slideo_matcher_set_frame_shading(tap._h, 65, 33, 24, p(g)) == 1 and L.slideo_matcher_set_frame_shading(tap._h, 0, 33, 16, p(g)) == 1
    assert L.slideo_matcher_set_frame_shading(tap._h, 4097, 33, 16, p(g)) == 1
    assert np.array_equal(tap.frame_shading()[3], g)
    tap.set_frame_shading(gains=None)
    assert L.slideo_matcher_frame_shading(tap._h, p(few), C.c_int64(4), *[C.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [0, 0, 0, 0] and (few == 9).all()


# ---- 2. every call form under a field equals its default twin on the shaded images -----------------------------------------------------

@pytest.fixture(scope="module")
def deck(cfg0_data):
    pages, frames, _, _ = cfg0_data
    return pages, np.ascontiguousarray(np.repeat(frames, 2, axis=0))      # every frame twice: changed and unchanged flags both occur


def _matcher(capi, pages, field=None, sift=None):
    m = capi.Matcher(small_cfg(capi))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if field is not None:
        m.set_frame_shading(*field)
    return m


@pytest.fixture(scope="module", params=[16, 32, 64])
def pair(request, capi, deck):
    """A matcher under the field, a matcher under the default, the sequence and the restatement's shaded images of it."""
    cell = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    g = _vignette(w, h, cell)
    m, ref = _matcher(capi, pages, (w, h, cell, g)), _matcher(capi, pages)
    yield cell, g, m, ref, seq, R.apply(seq, cell, g), w, h
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
    cell, g, m, ref, seq, sha, w, h = pair
    n = len(seq)
    want = ref.match_frames(sha)
    c_want = [ref.last_candidates(i) for i in range(n)]
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
    c, _ = _code(capi, lambda: m.set_frame_shading(gains=None))   # a busy matcher refuses the setter, and the field stays
    assert c == 4 and np.array_equal(m.frame_shading()[3], g)
    got += [m.collect(t_) for t_ in pend]
    assert _same(np.concatenate(got), want)
    assert _untouched(t, 0, host)


def test_with_a_levels_table_one_pass_does_both(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    m.set_frame_levels(MILD_LUT)
    try:
        both = LR.apply(sha, MILD_LUT)
        want = ref.match_frames(both)
        assert _same(m.match_frames(seq), want)
        t, p, stride, fs, host = _device_frames(seq, 1, 4, 8)
        assert _same(m.match_frames_dev(p, len(seq), w, h, stride, fs), want) and _untouched(t, 1, host)
        assert np.array_equal(m.shading_bgr(seq[0]), both[0]) and np.array_equal(m.levels_bgr(seq[0]), LR.apply(seq[0], MILD_LUT))
        ch, sim, last = ref.changed_mask(both)
        gc, gs, gl = m.changed_mask(seq)
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        m.set_frame_levels(None)


def test_changed_mask_and_kept_frames_are_not_shaded_twice(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    ch, sim, last = ref.changed_mask(sha)
    assert ch.any() and not ch.all()
    kept_want = ref.match_kept_frames([0, 3, 4])
    gc, gs, gl = m.changed_mask(seq)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    # (a second pass of the field would be another picture: the twin on twice-shaded frames differs)
    assert not _same(ref.match_frames(R.apply(sha, cell, g)[[0, 3, 4]]), kept_want)


@pytest.mark.parametrize("gate", ["previous", "anchor_settle"])
def test_gated_calls(capi, pair, gate):
    cell, g, m, ref, seq, sha, w, h = pair
    n = len(seq)
    for x in (m, ref):
        if gate != "previous":
            x.set_gate_reference("anchor")
            x.set_gate_settle(0.99, 2)
        x.gate_reset()
    try:
        want = [ref.match_changed_frames(sha[:5]), ref.match_changed_frames(sha[5:])]
        got = [m.match_changed_frames(seq[:5]), m.match_changed_frames(seq[5:])]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1])
        assert np.array_equal(m.gate_last_small(), ref.gate_last_small())
        assert m.gate_state_export() == ref.gate_state_export()
        t, p, stride, fs, host = _device_frames(seq, 1, 4, 8)
        m.gate_reset()
        got = [m.match_changed_frames_dev(p, 5, w, h, stride, fs), m.match_changed_frames_dev(p + 5 * fs, n - 5, w, h, stride, fs)]
        assert _same3(got[0], want[0]) and _same3(got[1], want[1]) and m.gate_state_export() == ref.gate_state_export()
        ref.gate_reset_from_frame(sha[2])
        a = ref.match_changed_frames(sha[3:6])
        m.gate_reset_from_frame(seq[2])
        assert _same3(m.match_changed_frames(seq[3:6]), a)
        m.gate_reset_from_frame_dev(p + 2 * fs, w, h, stride)
        assert _same3(m.match_changed_frames_dev(p + 3 * fs, 3, w, h, stride, fs), a)
        # slideo_matcher_gate_reset(small) is untouched: the small image is taken as it is
        small = ref.gate_last_small()
        for x in (m, ref):
            x.gate_reset(small)
        assert m.gate_state_export() == ref.gate_state_export()
        assert _untouched(t, 1, host)
    finally:
        for x in (m, ref):
            x.set_gate_settle(0, 0)
            x.set_gate_reference("previous")
            x.gate_reset()


def test_observe_frames_and_the_sessions_see_shaded_frames(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    for x, f in ((ref, sha), (m, seq)):
        x.activity_begin(12)
        x.content_begin(24)
        x.levels_begin()
        x.observe_frames(f[:7])
    t, p, stride, fs, host = _device_frames(seq, 2, 0, 3)
    m.observe_frames_dev(p + 7 * fs, 3, w, h, stride, fs)
    ref.observe_frames(sha[7:10])
    a, b = m.activity_counts(), ref.activity_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 9 and b[0].any()
    a, b = m.content_counts(), ref.content_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 10
    assert np.array_equal(m.levels_histogram(), ref.levels_histogram())
    assert _untouched(t, 2, host)
    for x in (m, ref):
        x.activity_end(); x.content_end(); x.levels_end()
    # the match sessions: evidence, tone and placement counts of the shaded frames
    for x, f in ((ref, sha), (m, seq)):
        x.evidence_begin(32, 8)
        x.tone_begin(8, 8, 255)
        x.placement_begin(32, 8, 6.0)
        x.match_frames(f)
    for name in ("evidence_counts", "tone_counts", "placement_sums"):
        a, b = getattr(m, name)(), getattr(ref, name)()
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v)), name
    # the setter ends them, as every setter that changes the analysed image does
    m.set_frame_shading(w, h, cell, g)
    for name in ("evidence_info", "tone_info", "placement_info"):
        assert _code(capi, getattr(m, name))[0] == 4
    for x in (ref,):
        x.evidence_end(); x.tone_end(); x.placement_end()


def test_frame_features_tap_and_the_untouched_taps(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    sel = [1, 2, 6]
    feats = [ref.orb(sha[i]) for i in sel]                        # (the single-image tap is untouched: the shaded image's features)
    kps, descs = [f[0] for f in feats], [f[1] for f in feats]
    want = ref.match_features(sha[sel], kps, descs)
    assert _same(m.match_features(seq[sel], kps, descs), want)
    assert np.array_equal(m.orb(seq[1])[1], ref.orb(seq[1])[1])   # pages and single-image taps do not see the field
    assert np.array_equal(m.levels_bgr(seq[1]), seq[1])


def test_under_a_working_size_a_region_and_another_pixel_format(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    t, p, stride, fs, host = _device_frames(seq, 0, 4, 0)
    g2 = _vignette(480, 270, cell)
    # a working size: the field of the reduce tap's image; the 640x360 field refuses frames analysed at 480x270
    m.set_working_size(480, 270)
    try:
        c, msg = _code(capi, lambda: m.match_frames(seq[:2]))
        assert c == 1 and "480x270" in msg and "640x360" in msg
        assert _code(capi, lambda: m.match_changed_frames(seq[:2]))[0] == 1
        m.set_frame_shading(480, 270, cell, g2)
        red6 = np.stack([ref.reduce(seq[i], 480, 270) for i in range(6)])
        want = ref.match_frames(R.apply(red6, cell, g2))
        assert _same(m.match_frames(seq[:6]), want)
        assert _same(m.match_frames_dev(p, 6, w, h, stride, fs), want)
        ch, sim, last = ref.changed_mask(R.apply(red6, cell, g2))
        gc, gs, gl = m.changed_mask(seq[:6])
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        m.set_working_size(0, 0)
    # a frame region: the field of the rectify tap's image
    quad = [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)]
    m.set_frame_region(w, h, quad, 480, 270)
    ref.set_frame_region(w, h, quad, 480, 270)
    try:
        rect = np.stack([ref.rectify(seq[i]) for i in range(6)])
        assert np.array_equal(m.rectify(seq[0]), rect[0])         # the rectify tap shows the image in front of the field
        ref.clear_frame_region()
        srect = R.apply(rect, cell, g2)
        assert _same(m.match_frames(seq[:6]), ref.match_frames(srect))
        for x in (m, ref):
            x.gate_reset()
        a = ref.match_changed_frames(srect)
        assert _same3(m.match_changed_frames(seq[:6]), a)
        m.gate_reset()
        assert _same3(m.match_changed_frames_dev(p, 6, w, h, stride, fs), a)
    finally:
        for x in (m, ref):
            x.clear_frame_region()
            x.gate_reset()
        m.set_frame_shading(w, h, cell, g)
    assert _untouched(t, 0, host)
    # another pixel format: the field comes behind the conversion
    m.set_pixel_format("rgba")
    try:
        rgba = np.concatenate([seq[:6, :, :, ::-1], np.full((6, h, w, 1), 99, np.uint8)], axis=3)
        assert np.array_equal(m.pixels_to_bgr(rgba[0]), seq[0])   # the conversion tap shows the image in front of the field
        assert _same(m.match_frames(rgba), ref.match_frames(sha[:6]))
    finally:
        m.set_pixel_format("bgr")


def test_the_yuv_door(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = np.random.default_rng(1).integers(16, 236, (4, fb), dtype=np.uint8)
    yuv[2] = yuv[1]
    imgs = np.stack([ref.yuv420_to_bgr(yuv[i], w, h, L) for i in range(4)])
    assert np.array_equal(m.yuv420_to_bgr(yuv[0], w, h, L), imgs[0])      # the conversion tap: in front of the field
    simgs = R.apply(imgs, cell, g)
    assert _same(m.match_frames_yuv420(yuv, w, h, L), ref.match_frames(simgs))
    for x in (m, ref):
        x.gate_reset()
    got, want = m.match_changed_frames_yuv420(yuv, w, h, L), ref.match_changed_frames(simgs)
    assert _same3(got, want) and np.array_equal(m.gate_last_small(), ref.gate_last_small())
    for x in (m, ref):
        x.gate_reset()


def test_sift_mode(capi, deck):
    pages, seq = deck
    n, h, w, _ = seq.shape
    g = _vignette(w, h, 32)
    sift = (capi.sift_config(nfeatures=300), 0.0)
    m, ref = _matcher(capi, pages, (w, h, 32, g), sift), _matcher(capi, pages, None, sift)
    sel = seq[::3]
    want = ref.match_frames(R.apply(sel, 32, g))
    assert (want["page_idx"] >= 0).any()
    assert _same(m.match_frames(sel), want)
    for i in range(len(sel)):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    m.close(); ref.close()


def test_group_of_two_members(capi, pair, deck):
    cell, g, m, ref, seq, sha, w, h = pair
    want = ref.match_frames(sha)
    ch, sim, last = ref.changed_mask(sha)
    kept = ref.match_kept_frames([1, 2, 9])
    ref.gate_reset()
    gated = ref.match_changed_frames(sha)
    ref.gate_reset()
    grp = capi.Group(small_cfg(capi), [0, 0])
    grp.add_pages(list(deck[0]))
    grp.finalize()
    grp.set_frame_shading(w, h, cell, g)
    assert np.array_equal(grp.frame_shading()[3], g)
    assert _same(grp.match_frames(seq), want)
    gc, gs, gl = grp.changed_mask(seq)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(grp.match_kept_frames([1, 2, 9]), kept)
    assert _same3(grp.match_changed_frames(seq), gated)
    on = [C.c_int32() for _ in range(4)]
    m1 = C.c_void_p(capi.lib().slideo_group_member(grp._h, 1))
    assert capi.lib().slideo_matcher_frame_shading(m1, None, C.c_int64(0), *[C.byref(x) for x in on]) == 0 and on[3].value == 1
    # a refused field changes no member
    bad = g.copy(); bad[0, 0] = 0
    with pytest.raises(ValueError):
        grp.set_frame_shading(w, h, 24, g)
    assert capi.lib().slideo_group_set_frame_shading(grp._h, w, h, 24, g.ctypes.data_as(C.c_void_p)) == 1
    assert capi.lib().slideo_group_set_frame_shading(grp._h, w, h, cell, bad.ctypes.data_as(C.c_void_p)) == 1
    assert np.array_equal(grp.frame_shading()[3], g)
    grp.close()


# ---- 3. the state a set call leaves --------------------------------------------------------------------------------------------------

def test_setting_ends_the_kept_frames_and_resets_the_gate(capi, pair):
    cell, g, m, ref, seq, sha, w, h = pair
    m.changed_mask(seq[:4])
    assert len(m.match_kept_frames([0, 1])) == 2
    m.gate_reset()
    m.match_changed_frames(seq[:2])
    assert m.gate_last_small().ndim == 3
    m.changed_mask(seq[:4])
    m.set_frame_shading(w, h, cell, g)                            # (the same field: a set call all the same)
    assert _code(capi, lambda: m.match_kept_frames([0]))[0] == 4   # SLIDEO_ERR_STATE: no kept frames
    assert _code(capi, lambda: m.gate_last_small())[0] == 4        # the gate state is "none"
    ch, _, _ = m.match_changed_frames(seq[1:3])
    assert ch[0]
    m.gate_reset()
    # off and on again: the default's bytes, then the field's
    m.set_frame_shading(gains=None)
    assert _same(m.match_frames(seq[:4]), ref.match_frames(seq[:4]))
    m.set_frame_shading(w, h, cell, R.identity(w, h, cell))       # the identity is stored as off
    assert m.frame_shading() is None and _same(m.match_frames(seq[:4]), ref.match_frames(seq[:4]))
    m.set_frame_shading(w, h, cell, g)
    assert _same(m.match_frames(seq[:4]), ref.match_frames(sha[:4]))
