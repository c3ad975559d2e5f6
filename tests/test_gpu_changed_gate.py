"""The changed-frame gate (include/slideo_amd.h "Changed-frame gate") against the EXISTING pair, on a second matcher of the same
config: one changed_mask call over the whole sequence, then match_frames of the flagged frames.  Every comparison is exact equality
of bytes: flags, similarities, verdicts of changed frames, the (-1, 0, 0, 0) record of unchanged ones, candidate traces, the last
small image.  The gated path's own output is never the reference.

Sequences (`_lecture`): synthetic lecture streams of slideo_amd.synth frames — holds of identical frames (SSD 0), holds whose
frames differ from the hold's first in three pixels (a tiny SSD: unchanged), and page changes.  Frame 64 starts a hold and frames
32, 96 and 128 lie inside holds by construction, so that unit boundaries of 32- and 64-frame units fall on a change and inside a
hold; `_conditions` asserts this, on the REFERENCE's flags, before anything is compared.
"""
import os

import numpy as np
import pytest

import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
UNCHANGED = (-1, 0.0, 0, 0)


def _lecture(synth, pages, n, w=640, h=360, seed=11, starts_at=(64,), inside=(32, 96, 128)):
    """-> (frames [n, h, w, 3], starts: the first frame of every hold)."""
    rng = np.random.default_rng(seed)
    starts, i = [0], 0
    while True:
        i += int(rng.integers(1, 13))
        if i >= n:
            break
        starts.append(i)
    starts = sorted((set(starts) | {s for s in starts_at if s < n}) - {s for s in inside})
    base, truth, _ = synth.frames(pages, len(starts), w, h, threads=NCPU)
    # consecutive holds must show different images: drop the rare repeat of a "no slide" frame by keeping the synthetic order
    seq = np.empty((n, h, w, 3), np.uint8)
    for j, s in enumerate(starts):
        e = starts[j + 1] if j + 1 < len(starts) else n
        seq[s:e] = base[j]
        if j % 3 == 1:                                            # a hold with a few altered pixels
            for t in range(s + 1, e):
                ys, xs = rng.integers(0, h, 3), rng.integers(0, w, 3)
                seq[t, ys, xs] ^= 0x55
    return seq, np.array(starts)


def _conditions(changed, starts, units):
    """What a sequence must show on the reference's flags; a sequence that does not is a failure of the test, not a skip."""
    assert changed.any() and not changed.all()
    assert changed[starts].all(), "the first frame of every page change is flagged"
    for u in units:
        b = np.arange(u, len(changed), u)
        assert len(b) and (~changed[b]).any() and changed[b].any(), "unit size %d: a boundary inside a hold and one on a change" % u


def _matcher(capi, pages, cfg=None, ws=None, sift=None):
    m = capi.Matcher(cfg if cfg is not None else small_cfg(capi))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if ws:
        m.set_working_size(*ws)
    return m


class Ref:
    """The existing pair on matcher r: flags, similarities, last small image, verdicts and traces of the flagged frames."""

    def __init__(self, r, seq, prev_small=None, yuv=None):
        if yuv is None:
            self.changed, self.sims, self.last = r.changed_mask(seq, prev_small)
        else:
            w, h, L = yuv
            self.changed, self.sims, self.last = r.changed_mask_yuv420(seq, w, h, L, prev_small)
        self.idx = np.nonzero(self.changed)[0]
        if len(self.idx):
            self.v = r.match_frames(seq[self.idx]) if yuv is None else r.match_frames_yuv420(seq[self.idx], yuv[0], yuv[1], yuv[2])
        else:
            self.v = np.zeros(0, capi_verdict_dtype(r))
        self.traces = [r.last_candidates(k).tobytes() for k in range(len(self.idx))]


def capi_verdict_dtype(m):
    from slideo_amd import _capi
    return _capi.VERDICT_DTYPE


def _equal(ref, got, lo=0, hi=None, what=""):
    """A gated result over frames [lo, hi) of the reference's sequence."""
    changed, sims, v = got
    hi = len(ref.changed) if hi is None else hi
    assert len(changed) == hi - lo, what
    assert np.array_equal(changed, ref.changed[lo:hi]), (what, np.nonzero(changed != ref.changed[lo:hi])[0][:8])
    assert sims.tobytes() == ref.sims[lo:hi].tobytes(), (what, np.nonzero(sims != ref.sims[lo:hi])[0][:8])
    k0 = int(ref.changed[:lo].sum())
    want = np.zeros(hi - lo, v.dtype)
    want[:] = UNCHANGED
    want[changed] = ref.v[k0:k0 + int(changed.sum())]
    assert v.tobytes() == want.tobytes(), (what, [i for i in range(hi - lo) if v[i] != want[i]][:8])


def _traces(ref, m, k0=0, count=None, what=""):
    count = len(ref.idx) - k0 if count is None else count
    for k in range(count):
        assert m.last_candidates(k).tobytes() == ref.traces[k0 + k], (what, "trace of changed frame %d" % (k0 + k))


def _stream(m, submit, n, unit, collect=None):
    """Gated submit / collect in units of `unit`, max_in_flight at once, in order -> the concatenated result."""
    collect = collect or m.collect_changed
    got, pend = [], []
    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            got.append(collect(pend.pop(0)))
        pend.append(submit(i, min(unit, n - i)))
    got += [collect(t) for t in pend]
    return tuple(np.concatenate([g[j] for g in got]) for j in range(3))


@pytest.fixture(scope="module")
def lecture(capi, synth):
    pages = synth.pages(4, 800, 450)
    seq, starts = _lecture(synth, pages, 192)
    r = _matcher(capi, pages)
    ref = Ref(r, seq)
    r.close()
    _conditions(ref.changed, starts, (1, 7, 32, 64))
    return pages, seq, starts, ref


@pytest.fixture(scope="module")
def lecture_yuv(capi, lecture):
    """The same stream as packed NV12 and I420, each with its own reference (the conversion is lossy: other flags may result)."""
    pages, seq, starts, _ = lecture
    h, w = seq.shape[1:3]
    out = {}
    for fmt in ("nv12", "i420"):
        L, fb = capi.yuv420_layout(fmt, w, h)
        yuv = yref.frames_to_yuv(seq, L, fb)
        r = _matcher(capi, pages)
        ref = Ref(r, yuv, yuv=(w, h, L))
        r.close()
        _conditions(ref.changed, starts, (1, 7, 32, 64))
        out[fmt] = (yuv, L, ref)
    return out


CUTS = (0, 50, 51, 64, 130, 192)        # several calls that continue the gate: a one-frame call, a cut on a change, cuts inside holds


def test_host_bgr_one_call_and_several(capi, lecture):
    pages, seq, _, ref = lecture
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames(seq), what="one call")
    _traces(ref, m, what="one call")
    assert np.array_equal(m.gate_last_small(), ref.last)
    m.gate_reset(None)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        _equal(ref, m.match_changed_frames(seq[lo:hi]), lo, hi, "call %d..%d" % (lo, hi))
        _traces(ref, m, int(ref.changed[:lo].sum()), int(ref.changed[lo:hi].sum()), "call %d..%d" % (lo, hi))
    assert np.array_equal(m.gate_last_small(), ref.last)
    m.close()


def test_host_pinned_bgr(capi, lecture):
    """A page-locked source: the ordered copy stream, host units of 32."""
    import torch
    pages, seq, _, ref = lecture
    pin = torch.empty(seq.shape, dtype=torch.uint8, pin_memory=True)
    pin.copy_(torch.from_numpy(seq))
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames(pin.numpy()), what="pinned")
    _traces(ref, m, what="pinned")
    m.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_host_yuv420_one_call_and_several(capi, lecture, lecture_yuv, fmt):
    pages, seq, _, _ = lecture
    h, w = seq.shape[1:3]
    yuv, L, ref = lecture_yuv[fmt]
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames_yuv420(yuv, w, h, L), what=fmt)
    _traces(ref, m, what=fmt)
    assert np.array_equal(m.gate_last_small(), ref.last)
    m.gate_reset(None)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        _equal(ref, m.match_changed_frames_yuv420(yuv[lo:hi], w, h, L), lo, hi, "%s call %d..%d" % (fmt, lo, hi))
    assert np.array_equal(m.gate_last_small(), ref.last)
    m.close()


def test_device_bgr_sync_and_streaming(capi, lecture):
    """Device BGR as one call, as several calls, and submit / collect with four units in flight at unit sizes 1, 7 and 64."""
    import torch
    pages, seq, _, ref = lecture
    n, h, w, _ = seq.shape
    d = torch.from_numpy(seq).cuda()
    fb = w * h * 3
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames_dev(d.data_ptr(), n, w, h), what="dev one call")
    _traces(ref, m, what="dev one call")
    m.gate_reset(None)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        _equal(ref, m.match_changed_frames_dev(d.data_ptr() + lo * fb, hi - lo, w, h), lo, hi, "dev call %d..%d" % (lo, hi))
    for unit in (1, 7, 64):
        m.gate_reset(None)
        got = _stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fb, c, w, h), n, unit)
        _equal(ref, got, what="stream unit %d" % unit)
        _traces(ref, m, what="stream unit %d" % unit)      # (the matcher is never idle between the units: the traces accumulate)
        assert np.array_equal(m.gate_last_small(), ref.last)
    m.close()


def test_device_pitched_bgr(capi, lecture):
    """Caller memory with a row pitch and a frame gap: the gather's row path."""
    import torch
    pages, seq, _, ref = lecture
    n, h, w, _ = seq[:96].shape
    stride, fs = w * 3 + 21, (w * 3 + 21) * h + 4          # rows at every alignment: the gather's 16-byte, 4-byte and byte paths
    buf = np.random.default_rng(3).integers(0, 256, (n, fs), dtype=np.uint8)
    for i in range(n):
        buf[i, :stride * h].reshape(h, stride)[:, :w * 3] = seq[i].reshape(h, w * 3)
    d = torch.from_numpy(buf).cuda()
    m = _matcher(capi, pages)
    got = _stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fs, c, w, h, stride, fs), n, 7)
    _equal(ref, got, 0, n, "pitched")
    m.close()


def test_device_nv12_sync_and_streaming(capi, lecture, lecture_yuv):
    import torch
    pages, seq, _, _ = lecture
    n, h, w, _ = seq.shape
    yuv, L, ref = lecture_yuv["nv12"]
    fs = yuv.shape[1]
    d = torch.from_numpy(yuv).cuda()
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames_yuv420_dev(d.data_ptr(), n, w, h, L, fs), what="nv12 dev")
    m.gate_reset(None)
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        _equal(ref, m.match_changed_frames_yuv420_dev(d.data_ptr() + lo * fs, hi - lo, w, h, L, fs), lo, hi, "nv12 dev %d..%d" % (lo, hi))
    m.gate_reset(None)
    got = _stream(m, lambda i, c: m.submit_changed_yuv420_dev(d.data_ptr() + i * fs, c, w, h, L, fs), n, 7)
    _equal(ref, got, what="nv12 stream")
    _traces(ref, m, what="nv12 stream")
    assert np.array_equal(m.gate_last_small(), ref.last)
    m.close()


def test_units_without_and_with_only_changed_frames_and_one_frame(capi, lecture):
    import torch
    pages, seq, starts, ref = lecture
    n, h, w, _ = seq.shape
    fb = w * h * 3
    d = torch.from_numpy(seq).cuda()
    m = _matcher(capi, pages)
    # a hold of at least 4 frames: frames 1.. of it as one unit hold no changed frame
    lens = np.diff(np.append(starts, n))
    j = int(np.argmax(lens))
    s, e = int(starts[j]), int(starts[j] + lens[j])
    assert e - s >= 4 and not ref.changed[s + 1:e].any()
    m.gate_reset(None)
    _equal(ref, m.match_changed_frames_dev(d.data_ptr(), s + 1, w, h), 0, s + 1, "head")
    t = m.submit_changed_dev(d.data_ptr() + (s + 1) * fb, e - s - 1, w, h)
    _equal(ref, m.collect_changed(t), s + 1, e, "a unit with no changed frame")
    # all frames changed: the first frames of the holds, against a reference of their own
    firsts = np.ascontiguousarray(seq[starts[:16]])
    r = _matcher(capi, pages)
    ref2 = Ref(r, firsts)
    r.close()
    assert ref2.changed.all()
    m.gate_reset(None)
    df = torch.from_numpy(firsts).cuda()
    _equal(ref2, m.collect_changed(m.submit_changed_dev(df.data_ptr(), len(firsts), w, h)), what="a unit with all frames changed")
    _traces(ref2, m, what="all changed")
    # n == 1, first as a changed frame (state none), then the same frame again (unchanged)
    m.gate_reset(None)
    _equal(ref, m.match_changed_frames(seq[:1]), 0, 1, "n == 1")
    got = m.match_changed_frames(seq[:1])
    assert not got[0][0] and got[1][0] == np.float32(1.0) and tuple(got[2][0]) == UNCHANGED
    m.close()


def test_gate_reset_with_a_small_image(capi, lecture):
    pages, seq, _, ref = lecture
    r = _matcher(capi, pages)
    small0 = r.changed_mask(seq[:1])[2]                      # frame 0's small image
    other = r.changed_mask(seq[70:71])[2]
    assert not np.array_equal(small0, other)
    m = _matcher(capi, pages)
    for prev in (small0, other):
        want = Ref(r, seq[:40], prev_small=prev)
        m.gate_reset(prev)
        assert np.array_equal(m.gate_last_small(), prev)
        _equal(want, m.match_changed_frames(seq[:40]), what="reset with a small image")
        assert np.array_equal(m.gate_last_small(), want.last)
    want = Ref(r, seq[:40], prev_small=small0)
    assert not want.changed[0] and want.sims[0] == np.float32(1.0)
    assert Ref(r, seq[:40], prev_small=other).changed[0]
    m.gate_reset(None)
    with pytest.raises(capi.SlideoError) as e:
        m.gate_last_small()
    assert e.value.code == 4
    r.close(); m.close()


def _option_case(capi, synth, pages, seq, cfg=None, ws=None, sift=None, page_set=None, units=(7,)):
    import torch
    r = _matcher(capi, pages, cfg() if cfg else None, ws, sift)
    m = _matcher(capi, pages, cfg() if cfg else None, ws, sift)
    if page_set is not None:
        r.use_page_set(r.create_page_set(page_set))
        m.use_page_set(m.create_page_set(page_set))
    ref = Ref(r, seq)
    assert ref.changed.any() and not ref.changed.all()
    assert (ref.v["page_idx"] >= 0).any(), "the reference assigns a page to some changed frame"
    _equal(ref, m.match_changed_frames(seq), what="host")
    _traces(ref, m, what="host")
    assert np.array_equal(m.gate_last_small(), ref.last)
    n, h, w, _ = seq.shape
    d = torch.from_numpy(seq).cuda()
    for unit in units:
        m.gate_reset(None)
        got = _stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * w * h * 3, c, w, h), n, unit)
        _equal(ref, got, what="stream %d" % unit)
        _traces(ref, m, what="stream %d" % unit)
    r.close(); m.close()
    return ref


@pytest.mark.parametrize("mode", ["verify_model_1", "ratio_test", "matcher_1", "page_set"])
def test_matcher_options(capi, synth, lecture, mode):
    pages, seq, _, _ = lecture
    cfgs = {"verify_model_1": lambda: small_cfg(capi, verify_model=1), "ratio_test": lambda: small_cfg(capi, ratio_test=0.9),
            "matcher_1": lambda: small_cfg(capi, matcher=1), "page_set": None}
    _option_case(capi, synth, pages, seq[:80], cfg=cfgs[mode], page_set=[0, 2] if mode == "page_set" else None)


def test_sift_mode(capi, synth):
    pages = synth.pages(3, 800, 450)
    seq, _ = _lecture(synth, pages, 24, seed=5, starts_at=(), inside=())
    _option_case(capi, synth, pages, seq, sift=(capi.sift_config(nfeatures=300), 0.0), units=(5,))


def test_working_size_on_4k_frames(capi, synth):
    pages = synth.pages(4, threads=NCPU)
    seq, _ = _lecture(synth, pages, 14, 3840, 2160, seed=2, starts_at=(), inside=())
    ref = _option_case(capi, synth, pages, seq, cfg=lambda: capi.default_config(nfeatures=1000), ws=(1920, 1080), units=(4,))
    assert ref.last.shape[:2] == capi.small_size(1920, 1080, 120000)[::-1]      # the small image is the REDUCED image's


def test_gated_and_plain_units_in_flight_together(capi, lecture):
    import torch
    pages, seq, _, ref = lecture
    n, h, w, _ = seq[:64].shape
    fb = w * h * 3
    d = torch.from_numpy(seq).cuda()
    r = _matcher(capi, pages)
    plain_want = r.match_frames(seq[100:110])
    r.close()
    m = _matcher(capi, pages)
    t1 = m.submit_changed_dev(d.data_ptr(), 20, w, h)
    tp = m.submit_dev(d.data_ptr() + 100 * fb, 10, w, h)              # does not touch the gate state
    t2 = m.submit_changed_dev(d.data_ptr() + 20 * fb, 44, w, h)
    # the wrong collect for a ticket, a collect out of order: SLIDEO_ERR_STATE, and the units stay in flight
    for bad in (lambda: m.collect(t1), lambda: m.collect_changed(tp), lambda: m.collect_changed(t2)):
        with pytest.raises(capi.SlideoError) as e:
            bad()
        assert e.value.code == 4
    _equal(ref, m.collect_changed(t1), 0, 20, "gated 1")
    with pytest.raises(capi.SlideoError) as e:
        m.collect_changed(tp)
    assert e.value.code == 4
    assert m.collect(tp).tobytes() == plain_want.tobytes()
    _equal(ref, m.collect_changed(t2), 20, 64, "gated 2")
    m.close()


def test_size_change_without_a_reset_is_a_state_error(capi, synth, lecture):
    pages, seq, _, ref = lecture
    m = _matcher(capi, pages)
    _equal(ref, m.match_changed_frames(seq[:10]), 0, 10)
    other = synth.frames(pages, 2, 800, 450)[0]
    h, w = seq.shape[1:3]
    L, fb = capi.yuv420_layout("nv12", w, h)
    for bad in (lambda: m.match_changed_frames(other),
                lambda: m.match_changed_frames_yuv420(yref.frames_to_yuv(seq[:2], L, fb), w, h, L)):      # another size, another family
        with pytest.raises(capi.SlideoError) as e:
            bad()
        assert e.value.code == 4
    with pytest.raises(capi.SlideoError) as e:                         # an argument error
        m.match_changed_frames(np.zeros((2, 0, 4, 3), np.uint8))
    assert e.value.code == 1
    _equal(ref, m.match_changed_frames(seq[10:30]), 10, 30, "the gate state is untouched by the refused calls")
    m.gate_reset(None)
    got = m.match_changed_frames(other)
    assert got[0][0]
    m.close()


@pytest.mark.parametrize("env", [("SLIDEO_ASYNC_SUBMIT", "0"), ("SLIDEO_RNG_STREAM_LEN", "512"), ("nfeatures", 40)])
def test_rerun_paths(capi, lecture, monkeypatch, env):
    """The exact-size path from the start (SLIDEO_ASYNC_SUBMIT=0), a unit re-run from its gathered frames because the pre-drawn
    RNG stream was too short (flag 4), and a small nfeatures, where keypoint ties at a retainBest threshold are the likeliest to
    exceed the capacity-sized path (flag 8: whether it fires is the data's matter; the results must be the pair's either way)."""
    import torch
    pages, seq, _, ref0 = lecture
    cfg = None
    if env[0] == "nfeatures":
        cfg = lambda: small_cfg(capi, nfeatures=40)
    else:
        monkeypatch.setenv(*env)
    r = _matcher(capi, pages, cfg() if cfg else None)
    m = _matcher(capi, pages, cfg() if cfg else None)
    sub = seq[:80]
    ref = Ref(r, sub)
    n, h, w, _ = sub.shape
    d = torch.from_numpy(sub).cuda()
    _equal(ref, m.match_changed_frames(sub), what=str(env))
    m.gate_reset(None)
    got = _stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * w * h * 3, c, w, h), n, 7)
    _equal(ref, got, what="stream " + str(env))
    _traces(ref, m, what="stream " + str(env))
    r.close(); m.close()


class _PairOnly:
    """A matcher with the gated entry points hidden: the task falls back to the mask + kept pair."""
    HIDDEN = ("match_changed_frames", "match_changed_frames_yuv420", "gate_reset", "member")

    def __init__(self, m):
        self._m = m

    def __getattr__(self, name):
        if name in self.HIDDEN:
            raise AttributeError(name)
        return getattr(self._m, name)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_video_task_equals_the_pair(tmp_path, capi, lecture, fmt):
    """HipVideoMatcher.match_images_with_video on a RawVideo / RawVideoYuv420: the same Matching list with and without the gate."""
    from slideo_amd import matching as mt
    pages, seq, _, _ = lecture
    n, h, w, _ = seq.shape
    vid = os.path.join(tmp_path, "v")
    if fmt == "bgr":
        mt.RawVideo.write(vid, seq, fps=0.2)                     # one sample per frame
    else:
        L, fb = capi.yuv420_layout(fmt, w, h)
        mt.RawVideoYuv420.write(vid, yref.frames_to_yuv(seq, L, fb), w, h, fps=0.2, fmt=fmt)
    images = ["page-%d" % i for i in range(len(pages))]
    out = []
    for hide in (False, True):
        m = _matcher(capi, pages)
        vm = mt.HipVideoMatcher(_PairOnly(m) if hide else m, images)
        assert (mt._gated_matcher(vm._m) is None) == hide
        task = vm.match_images_with_video(vid, mt.ProgressReporter(lambda a, b, c: None))
        out.append(task.process())
        m.close()
    assert len(out[0]) > 3 and any(x.image is not None for x in out[0])
    assert out[0] == out[1]
