"""Decoded YUV 4:2:0 frames (include/slideo_amd.h "YUV 4:2:0 frames"): the conversion kernel (csrc/yuv420.hip.h) is bit-exact
against the numpy restatement (tests/yuv420_ref.py), and every *_yuv420 call returns exactly what its *_bgr8 twin returns on
the converted BGR image — host, device, streaming, mask + kept frames, group, SIFT mode and the trait-surface mirror."""
import os

import numpy as np
import pytest

import yuv420_ref as ref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

FORMATS = ("nv12", "nv21", "i420", "yv12")
NCPU = min(16, os.cpu_count() or 1)


def _align(x, a):
    return -(-x // a) * a


def _pitched(capi, fmt, w, h):
    return capi.yuv420_layout(fmt, w, h, pitch=_align(w, 256), row_align=16)


def _yuv_of(capi, frames, fmt="nv12", pitched=False):
    """BGR frames -> (4:2:0 frames [n, frame_bytes], layout, the BGR image the library makes of them)."""
    n, h, w, _ = frames.shape
    L, fb = _pitched(capi, fmt, w, h) if pitched else capi.yuv420_layout(fmt, w, h)
    yuv = ref.frames_to_yuv(frames, L, fb)
    bgr = np.stack([ref.to_bgr(f, w, h, L) for f in yuv])
    return yuv, L, bgr


def _matcher(capi, pages, cfg=None):
    m = capi.Matcher(cfg if cfg is not None else small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    return m


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


@pytest.mark.parametrize("w,h", [(640, 360), (1920, 1080), (3840, 2160), (642, 362)])
@pytest.mark.parametrize("pitched", [False, True])
def test_conversion_tap_bit_exact(capi, tap, w, h, pitched):
    """All four formats, random full-range bytes (out-of-gamut and clamped values included), tight and decoder-pitched layouts."""
    rng = np.random.default_rng(w * 31 + h + int(pitched))
    for fmt in FORMATS:
        L, fb = _pitched(capi, fmt, w, h) if pitched else capi.yuv420_layout(fmt, w, h)
        buf = rng.integers(0, 256, fb, dtype=np.uint8)
        got = tap.yuv420_to_bgr(buf, w, h, L)
        want = ref.to_bgr(buf, w, h, L)
        assert np.array_equal(got, want), (fmt, w, h, pitched, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("w,h", [(6, 4), (18, 10)])
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_batch_of_two_with_a_frame_stride_of_2_mod_4(capi, tap, fmt, w, h):
    """Two device frames in the decoder-pitched layout, whose rows allow every wide load of the 4:2:0 kernel, read in place at a
    frame stride of fb (the wide loads) and of fb + 2 (2 mod 4: the host takes the wide loads away, and the second frame's rows
    start where no dword load may).  No call returns the converted pixels of a batch; the activity accumulator
    (tests/activity_ref.py) counts the pixels that differ between consecutive converted frames.  The same frame twice: none
    differs, so frame 1 is converted as frame 0 is, which the tap holds to the restatement.  Two different frames: the counts of the
    restatement's two images.  Which flags the host chose at such a stride is tests/test_yuv_args_golden.py's to pin ("pitched+2")."""
    import torch
    import activity_ref as A
    L, fb = _pitched(capi, fmt, w, h)
    assert fb % 8 == 0 and L.y_stride % 8 == 0 and L.uv_stride % 4 == 0
    rng = np.random.default_rng(w * 131 + h + len(fmt))
    f0, f1 = rng.integers(0, 256, fb, dtype=np.uint8), rng.integers(0, 256, fb, dtype=np.uint8)
    want0, want1 = ref.to_bgr(f0, w, h, L), ref.to_bgr(f1, w, h, L)
    assert np.array_equal(tap.yuv420_to_bgr(f0, w, h, L), want0)
    for fs in (fb, fb + 2):
        for delta, second, want_second in ((0, f0, want0), (255, f1, want1)):
            buf = rng.integers(0, 256, 2 * fs, dtype=np.uint8)       # (the bytes between and behind the frames are noise)
            buf[:fb], buf[fs:fs + fb] = f0, second
            d = torch.from_numpy(buf).cuda()
            assert d.data_ptr() % 8 == 0
            tap.activity_begin(delta)
            tap.observe_frames_yuv420_dev(d.data_ptr(), 2, w, h, L, fs)
            got = tap.activity_counts()
            tap.activity_end()
            want = A.counts(np.stack([want0, want_second]), delta)
            assert got[1] == want[1] == 1 and np.array_equal(got[0], want[0]), (fmt, w, h, fs, delta, np.argwhere(got[0] != want[0])[:4])
        assert not want[0].all() and want[0].any()       # (delta 255 splits random frames: a wrong second frame would show)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_match_frames_equal_bgr_and_oracle(capi, oracle, cfg0_data, fmt):
    from test_gpu_parity import _build_both, _compare_traces
    pages, frames, truth, _ = cfg0_data
    h, w = frames.shape[1:3]
    yuv, L, bgr = _yuv_of(capi, frames, fmt)
    m, db = _build_both(capi, oracle, small_cfg(capi), small_cfg(oracle), pages)
    v_bgr = m.match_frames(bgr)
    c_bgr = [m.last_candidates(i) for i in range(len(bgr))]
    v = m.match_frames_yuv420(yuv, w, h, L)
    assert _same(v, v_bgr)
    for i in range(len(bgr)):
        assert _same(m.last_candidates(i), c_bgr[i]), "candidate trace of frame %d" % i
    _compare_traces(m, db, bgr, v)                               # (the traces of the YUV call against the oracle on that BGR)
    assert (v["page_idx"] == truth).mean() >= 0.75
    m.close()


def test_device_and_streaming_paths(capi, synth, monkeypatch):
    """Pitched NV12 in torch device memory through match_frames_yuv420_dev and submit / collect, several units in flight (a small
    workspace budget cuts the calls into many units over all slots); a pinned-source host call of >= 2 host units."""
    import torch
    monkeypatch.setenv("SLIDEO_WS_GB", "0.3")
    pages = synth.pages(4, 800, 450)
    frames, _, _ = synth.frames(pages, 96, 640, 360, threads=NCPU)
    n, h, w, _ = frames.shape
    yuv, L, bgr = _yuv_of(capi, frames, "nv12", pitched=True)
    m = _matcher(capi, pages)
    want = m.match_frames(bgr)
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    d = torch.from_numpy(yuv).cuda()
    fs = yuv.shape[1]
    assert _same(m.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, fs), want)
    # streaming: units of 8, up to max_in_flight at once, collected in order
    got, pend = [], []
    for i in range(0, n, 8):
        if len(pend) == m.max_in_flight():
            got.append(m.collect(pend.pop(0)))
        pend.append(m.submit_yuv420_dev(d.data_ptr() + i * fs, min(8, n - i), w, h, L, fs))
    got += [m.collect(t) for t in pend]
    assert _same(np.concatenate(got), want)
    # pinned host source (the copy-stream path), 96 >= 2 * 32 frames
    pin = torch.empty(yuv.shape, dtype=torch.uint8, pin_memory=True)
    pin.copy_(torch.from_numpy(yuv))
    assert _same(m.match_frames_yuv420(pin.numpy(), w, h, L), want)
    m.close()


def test_changed_mask_and_kept_frames(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    h, w = frames.shape[1:3]
    seq = np.repeat(frames, 2, axis=0)                           # every frame twice: unchanged and changed flags both occur
    yuv, L, bgr = _yuv_of(capi, seq, "nv12", pitched=True)
    m = _matcher(capi, pages)
    ch, sim, last = m.changed_mask(bgr)
    ch2, sim2, last2 = m.changed_mask(bgr[3:], prev_small=last)
    sel = np.nonzero(ch2)[0]
    want_kept = m.match_frames(bgr[3:][sel])
    yc, ys, yl = m.changed_mask_yuv420(yuv, w, h, L)
    assert np.array_equal(yc, ch) and _same(ys, sim) and np.array_equal(yl, last)
    assert ch.any() and not ch.all()
    yc2, ys2, yl2 = m.changed_mask_yuv420(yuv[3:], w, h, L, prev_small=yl)
    assert np.array_equal(yc2, ch2) and _same(ys2, sim2) and np.array_equal(yl2, last2)
    assert _same(m.match_kept_frames(sel), want_kept)
    m.close()


def test_group_equals_single_matcher(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    h, w = frames.shape[1:3]
    seq = np.repeat(frames, 2, axis=0)
    yuv, L, bgr = _yuv_of(capi, seq, "i420", pitched=True)
    m = _matcher(capi, pages)
    want = m.match_frames(bgr)
    ch, sim, last = m.changed_mask(bgr)
    sel = np.nonzero(ch)[0]
    want_kept = m.match_frames(bgr[sel])
    m.close()
    for devs in ([0, 0], [0, 0, 0]):
        g = capi.Group(small_cfg(capi), devs)
        g.add_pages(list(pages))
        g.finalize()
        assert _same(g.match_frames_yuv420(yuv, w, h, L), want), devs
        gc, gs, gl = g.changed_mask_yuv420(yuv, w, h, L)
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last), devs
        assert _same(g.match_kept_frames(sel), want_kept), devs
        g.close()


def test_sift_mode(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    h, w = frames.shape[1:3]
    yuv, L, bgr = _yuv_of(capi, frames, "nv12")
    m = capi.Matcher(small_cfg(capi))
    m.use_sift(capi.sift_config(nfeatures=400), 0.75)
    m.add_pages(list(pages))
    m.finalize()
    want = m.match_frames(bgr)
    c_want = [m.last_candidates(i) for i in range(len(bgr))]
    assert _same(m.match_frames_yuv420(yuv, w, h, L), want)
    for i in range(len(bgr)):
        assert _same(m.last_candidates(i), c_want[i])
    m.close()


def test_1080p_against_gpu_bgr_path(capi, synth):
    """64 1080p NV12 frames against a 100-page deck (configs[1]'s ORB-1000): the YUV host call equals the BGR host call."""
    pages = synth.pages(100, threads=NCPU)
    frames, truth, _ = synth.frames(pages, 64, 1920, 1080, threads=NCPU)
    yuv, L, bgr = _yuv_of(capi, frames, "nv12", pitched=True)
    m = _matcher(capi, pages, capi.default_config(nfeatures=1000))
    want = m.match_frames(bgr)
    assert _same(m.match_frames_yuv420(yuv, 1920, 1080, L), want)
    assert (want["page_idx"] == truth).mean() >= 0.8
    m.close()


def test_errors(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    h, w = frames.shape[1:3]
    yuv, L, bgr = _yuv_of(capi, frames[:2], "nv12")
    m = _matcher(capi, pages)

    def code(fn):
        with pytest.raises(capi.SlideoError) as e:
            fn()
        return e.value.code, str(e.value)

    assert code(lambda: m.match_frames_yuv420(yuv, w - 1, h, L))[0] == 5                 # odd width: UNSUPPORTED
    assert code(lambda: m.changed_mask_yuv420(yuv, w, h - 1, L))[0] == 5                 # odd height
    assert code(lambda: m.yuv420_to_bgr(yuv[0], w + 1, h, L))[0] == 5

    def bad(**f):
        B = capi.Yuv420Layout.from_buffer_copy(L)
        for k, v in f.items():
            setattr(B, k, v)
        return B
    c, msg = code(lambda: m.match_frames_yuv420(yuv, w, h, bad(y_stride=w - 2)))
    assert c == 1 and "y_stride" in msg
    c, msg = code(lambda: m.match_frames_yuv420(yuv, w, h, bad(u_offset=w * 10, v_offset=w * 10 + 1)))
    assert c == 1 and "overlaps" in msg
    c, msg = code(lambda: m.match_frames_yuv420(yuv, w, h, bad(u_offset=w * h, v_offset=w * h + w * h // 8, uv_step=1, uv_stride=w // 2)))
    assert c == 1 and "overlaps" in msg                                                 # planar U and V on top of each other
    c, msg = code(lambda: m.match_frames_yuv420(np.ascontiguousarray(yuv[:, :-2]), w, h, L))
    assert c == 1 and "frame_stride" in msg
    assert code(lambda: m.match_frames_yuv420(yuv, w, h, bad(uv_step=3)))[0] == 1
    assert code(lambda: m.match_frames_yuv420(yuv, w, h, bad(uv_stride=w - 2)))[0] == 1
    # a mask -> kept sequence broken by another upload: SLIDEO_ERR_STATE, as for BGR
    m.changed_mask_yuv420(yuv, w, h, L)
    m.match_frames_yuv420(yuv, w, h, L)
    assert code(lambda: m.match_kept_frames([0]))[0] == 4
    m.changed_mask(bgr)
    m.match_frames_yuv420(yuv, w, h, L)
    assert code(lambda: m.match_kept_frames([0]))[0] == 4
    # device-resident 4:2:0 frames are converted into a slot's staging buffer as well (match and submit); device-resident BGR
    # frames are read where they are, and the kept frames stay usable
    import torch
    d_yuv, d_bgr = torch.from_numpy(yuv).cuda(), torch.from_numpy(bgr).cuda()
    m.changed_mask(bgr)
    m.match_frames_yuv420_dev(d_yuv.data_ptr(), len(yuv), w, h, L, yuv.shape[1])
    assert code(lambda: m.match_kept_frames([0]))[0] == 4
    m.changed_mask(bgr)
    m.collect(m.submit_yuv420_dev(d_yuv.data_ptr(), len(yuv), w, h, L, yuv.shape[1]))
    assert code(lambda: m.match_kept_frames([0]))[0] == 4
    m.changed_mask(bgr)
    want_kept = m.match_kept_frames([0, 1])
    m.changed_mask(bgr)
    m.match_frames_dev(d_bgr.data_ptr(), len(bgr), w, h)
    assert _same(m.match_kept_frames([0, 1]), want_kept)
    m.close()


def test_trait_surface_mirror_on_yuv420_video(tmp_path, capi, synth):
    """HipVideoMatcherTask.process on a RawVideoYuv420 gives the timeline it gives on a RawVideo of the converted frames."""
    from PIL import Image
    from slideo_amd import matching as mt
    from test_matching_mirror import Page
    pages = synth.pages(4, 800, 450)
    page_objs = []
    for i, p in enumerate(pages):
        path = os.path.join(tmp_path, "p-%d.png" % (i + 1))
        Image.fromarray(p[:, :, ::-1]).save(path)
        page_objs.append(Page(path, i + 1))
    frames, _, _ = synth.frames(pages, 6, 640, 360)
    seq = np.repeat(frames, 10, axis=0)
    outs = []
    for fmt in ("nv12", "i420"):
        yuv, L, bgr = _yuv_of(capi, seq, fmt)
        vy, vb = os.path.join(tmp_path, "v-%s.slvy" % fmt), os.path.join(tmp_path, "v-%s.slvf" % fmt)
        mt.RawVideoYuv420.write(vy, yuv, 640, 360, fps=1.0, fmt=fmt)
        mt.RawVideo.write(vb, bgr, fps=1.0)
        assert isinstance(mt.open_raw_video(vy), mt.RawVideoYuv420) and isinstance(mt.open_raw_video(vb), mt.RawVideo)
        rep = mt.ProgressReporter(lambda a, b, c: None)
        vm = mt.HipImageVideoMatcher(capi.default_config(nfeatures=500, min_rating=12.0)).create_video_matcher(page_objs, rep)
        a = [(x.video_time, x.video_frame_idx, x.image) for x in vm.match_images_with_video(vy, rep).process()]
        b = [(x.video_time, x.video_frame_idx, x.image) for x in vm.match_images_with_video(vb, rep).process()]
        assert a == b and len(a) >= 3, fmt
        outs.append(a)
