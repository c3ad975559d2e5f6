"""Working size (include/slideo_amd.h "Working size"): the reduce tap (csrc/reduce.hip.h) equals the CPU restatement
so_resize_area_bgr8_v bit for bit and lies within the float64 definition's bound; every frame call made under a working size
returns, byte for byte, what the same call without one returns on the tap's output.

Inputs of the end-to-end tests: 6 synthetic pages of 2001x1125 and the first frames of synth.frames that show a slide, at
3840x2160 (2x2 fast path), 2560x1440 (factor 4/3, the tap kernel) and 4096x2160 (-> 1920x1013), ORB-1000 and the default config
otherwise.  Every end-to-end test asserts that at least three quarters of the frames receive a page on the COMPARISON side (the call
without a working size on the reduced images).  The CPU restatement alone meets that on these inputs — pyoracle.PageDB.match_frames
on pyoracle.resize_area outputs of the very frames, pages assigned of frames (all equal to the synthetic truth unless noted):

    mode                      3840x2160   2560x1440   4096x2160
    default                   8 / 8       8 / 8       8 / 8
    verify_model 1            8 / 8       8 / 8       8 / 8
    ratio_test 0.9            6 / 8       6 / 8       6 / 8      (the six assigned equal the truth)
    matcher 1                 8 / 8       8 / 8       8 / 8
    SIFT (ratio 0), 4 frames  4 / 4       4 / 4       4 / 4

(The page-set test selects the pages the frames show, and the 4:2:0 tests read the converted images of the first four frames: the
restatement was not run on those two; their comparison sides carry the same assertion on the GPU.)
"""
import ctypes as C
import os

import numpy as np
import pytest

import f64_defs as D
from f64_checks import report

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
WS = (1920, 1080)
CFG = dict(nfeatures=1000)


def _slides(synth, pages, n, w, h):
    """The first n frames of the synthetic stream that show a slide."""
    fr, truth, _ = synth.frames(pages, 2 * n, w, h, threads=NCPU)
    keep = np.nonzero(truth >= 0)[0][:n]
    assert len(keep) == n
    return np.ascontiguousarray(fr[keep]), truth[keep]


@pytest.fixture(scope="module")
def deck(synth):
    pages = synth.pages(6, threads=NCPU)
    return pages, {"4k": _slides(synth, pages, 8, 3840, 2160), "qhd": _slides(synth, pages, 8, 2560, 1440)}


def _matcher(capi, pages, ws=None, sift=None, **kw):
    m = capi.Matcher(capi.default_config(**dict(CFG, **kw)))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if ws:
        m.set_working_size(*ws)
    return m


def _reduced(capi, m, frames, ws=WS):
    """The tap's output for frames [n, h, w, 3] under the working size ws."""
    h, w = frames.shape[1:3]
    dw, dh = capi.working_size(w, h, *ws)
    return np.stack([m.reduce(f, dw, dh) for f in frames])


def _trace(m, v):
    """A call's verdict records and candidate traces as raw bytes."""
    return v.tobytes(), [m.last_candidates(i).tobytes() for i in range(len(v))]


def _paged(v, n=None):
    """The condition of every end-to-end test: three quarters of the comparison side's frames receive a page."""
    got = int((v["page_idx"] >= 0).sum())
    assert 4 * got >= 3 * len(v), (got, len(v))
    return got


def _oracle_area(oracle, buf, w, h, stride, dw, dh, variant):
    out = np.empty((dh, dw, 3), np.uint8)
    rc = oracle.lib().so_resize_area_bgr8_v(buf.ctypes.data_as(C.c_void_p), w, h, stride, out.ctypes.data_as(C.c_void_p), dw, dh, variant)
    assert rc == 0, rc
    return out


# (w, h, dw, dh, stride or None): the 2x2 dword kernel (contiguous and pitched by a multiple of 8), the integer kernel (factor 3; an
# odd 2x2 whose pitch is not a multiple of 4: the byte path; factors 2 x 3), the tap kernel (4/3, 2.13, barely above 1, an odd pitched
# source), and results one row high through each of the three
TAP_SHAPES = [
    (3840, 2160, 1920, 1080, None),
    (2560, 1440, 1280, 720, None),
    (1280, 720, 640, 360, 1280 * 3 + 8),
    (2880, 1620, 960, 540, None),
    (2560, 1440, 1920, 1080, None),
    (4096, 2160, 1920, 1013, None),
    (1921, 1081, 1920, 1080, None),
    (1282, 722, 641, 361, 1282 * 3 + 1),
    (1283, 721, 960, 540, 1283 * 3 + 2),
    (1280, 720, 640, 240, None),
    (2560, 2, 1280, 1, None),
    (300, 3, 100, 1, None),
    (1000, 5, 750, 1, None),
    (640, 360, 640, 180, None),
]


@pytest.fixture(scope="module", params=[0, 1])
def tap(request, capi):
    m = capi.Matcher(capi.default_config(ocv_area=request.param, **CFG))
    yield m, request.param
    m.close()


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "%dx%d-%dx%d%s" % (s[0], s[1], s[2], s[3], "-pitched" if s[4] else ""))
def test_tap_equals_the_restatement(capi, oracle, synth, tap, shape):
    m, variant = tap
    w, h, dw, dh, stride = shape
    stride = stride or w * 3
    rng = np.random.default_rng(w * 7 + h * 3 + dw)
    pages = synth.pages(2, 800, 450)
    for kind in ("synthetic", "noise"):
        img = synth.frames(pages, 1, w, h, first=3)[0][0] if kind == "synthetic" else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)          # (the pitch bytes are noise: they must not be read)
        buf[:, :w * 3] = img.reshape(h, w * 3)
        want = _oracle_area(oracle, buf, w, h, stride, dw, dh, variant)
        got = m.reduce_pitched(buf, w, h, stride, dw, dh)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (kind, shape, variant, int((got != want).sum()), np.argwhere(got != want)[:4])


@pytest.mark.parametrize("shape", [(2560, 1440, 1920, 1080), (4096, 2160, 1920, 1013), (1921, 1081, 1920, 1080)],
                         ids=lambda s: "%dx%d-%dx%d" % s)
def test_tap_against_the_float64_definition(capi, synth, shape):
    """f64_checks.check_area's bound rule at an explicit target size: every channel within 0.5 + eta of the exact box mean
    (f64_defs.area_resize, float64 numpy) and equal to rint(mean) wherever the mean is farther than eta (area_eta) from a rounding
    boundary.  The sharpness guard (eta must not swallow the check) is stated on the boundary band itself: a rational factor puts
    many means EXACTLY on a boundary (4/3: every weight is a multiple of 1/16, so one mean in sixteen is x.5, where both
    neighbours are correct roundings), so the guard counts the channels within eta of a boundary that are not such exact ties
    (farther than 1e-9 from it): at most 1 % of all channels.  ocv.area 0: the variant area_eta is derived for."""
    w, h, dw, dh = shape
    m = capi.Matcher(capi.default_config(**CFG))
    src = synth.frames(synth.pages(2), 1, w, h, first=4)[0][0]
    got = m.reduce(src, dw, dh)
    m.close()
    mean, _, _ = D.area_resize(src, dw, dh)
    eta = D.area_eta(w, h, dw, dh)[:, :, None]
    dev = np.abs(got - mean)
    off = np.abs(mean - np.floor(mean) - 0.5)                    # distance from the rounding boundary
    far = off > eta
    swallowed = ~far & (off > 1e-9)
    exact = got == np.rint(mean)
    report("reduce", size="%dx%d->%dx%d" % shape, max_dev=float(dev.max()), eta_max=float(eta.max()), exact=float(exact.mean()),
           far=float(far.mean()), swallowed=float(swallowed.mean()))
    assert (dev <= 0.5 + eta).all(), dev.max()
    assert exact[far].all(), "%d channels away from a rounding boundary differ" % (~exact & far).sum()
    assert swallowed.mean() <= 0.01, swallowed.mean()


@pytest.mark.parametrize("key", ["4k", "qhd"])
def test_host_and_device_calls(capi, deck, key):
    import torch
    pages, sets = deck
    frames, truth = sets[key]
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages, WS), _matcher(capi, pages)
    assert mw.working_size == WS and m0.working_size == (0, 0)
    red = _reduced(capi, m0, frames)
    want = _trace(m0, m0.match_frames(red))
    v0 = np.frombuffer(want[0], capi.VERDICT_DTYPE)
    _paged(v0)
    assert (v0["page_idx"] == truth).mean() >= 0.75
    assert _trace(mw, mw.match_frames(frames)) == want, "pageable host frames"
    pin = torch.from_numpy(frames).pin_memory()
    assert _trace(mw, mw.match_frames(pin.numpy())) == want, "pinned host frames"
    d = torch.from_numpy(frames).cuda()
    assert _trace(mw, mw.match_frames_dev(d.data_ptr(), n, w, h)) == want, "device frames"
    # pitched device frames (rows and frames further apart than the image)
    stride = w * 3 + 64
    dp = torch.zeros((n, h + 1, stride), dtype=torch.uint8, device="cuda")
    dp[:, :h, :w * 3] = d.reshape(n, h, w * 3)
    torch.cuda.synchronize()                                     # (torch's fill and copy kernels run on its own stream; the call is given none)
    assert _trace(mw, mw.match_frames_dev(dp.data_ptr(), n, w, h, stride, stride * (h + 1))) == want, "pitched device frames"
    # frames still being produced on the caller's stream when the call is made: the call is given that stream and orders the
    # reduce behind it
    ts = torch.cuda.Stream()                                     # (a stream of its own: the null stream's handle is 0 = "none")
    with torch.cuda.stream(ts):
        dq = torch.zeros((n, h + 1, stride), dtype=torch.uint8, device="cuda")
        dq[:, :h, :w * 3] = d.reshape(n, h, w * 3)
    assert ts.cuda_stream != 0
    got = mw.match_frames_dev(dq.data_ptr(), n, w, h, stride, stride * (h + 1), stream=ts.cuda_stream)
    assert _trace(mw, got) == want, "device frames produced on the caller's stream"
    mw.close(); m0.close()


def test_many_host_units(capi, deck, monkeypatch):
    """A host call cut into several units over all slots (a small workspace budget), pinned: the copy-stream path."""
    import torch
    monkeypatch.setenv("SLIDEO_WS_GB", "0.6")
    monkeypatch.setenv("SLIDEO_HOST_UNIT", "2")
    pages, sets = deck
    frames, _ = sets["4k"]
    mw, m0 = _matcher(capi, pages, WS), _matcher(capi, pages)
    want = _trace(m0, m0.match_frames(_reduced(capi, m0, frames)))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == want
    assert _trace(mw, mw.match_frames(torch.from_numpy(frames).pin_memory().numpy())) == want
    mw.close(); m0.close()


def test_submit_collect_four_units_two_of_which_reduce(capi, deck):
    import torch
    pages, sets = deck
    f4k, fq = sets["4k"][0], sets["qhd"][0]
    mw, m0 = _matcher(capi, pages, WS), _matcher(capi, pages)
    r4k, rq = _reduced(capi, m0, f4k), _reduced(capi, m0, fq)
    # units: 4K (reduced), 1080p (fits: untouched), 1440p (reduced), 1080p (untouched)
    units_w = [f4k[:4], rq[4:], fq[:4], r4k[4:]]
    units_0 = [r4k[:4], rq[4:], rq[:4], r4k[4:]]
    assert mw.max_in_flight() >= 4

    def run(m, units):
        dev = [torch.from_numpy(np.ascontiguousarray(u)).cuda() for u in units]
        tickets = [m.submit_dev(d.data_ptr(), d.shape[0], d.shape[2], d.shape[1]) for d in dev]      # four in flight
        v = np.concatenate([m.collect(t) for t in tickets])
        return _trace(m, v)
    want = run(m0, units_0)
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert run(mw, units_w) == want
    mw.close(); m0.close()


def test_changed_mask_and_kept_frames(capi, deck):
    pages, sets = deck
    frames, _ = sets["4k"]
    seq = np.repeat(frames[:4], 2, axis=0)                       # every frame twice: unchanged and changed flags both occur
    mw, m0 = _matcher(capi, pages, WS), _matcher(capi, pages)
    red = _reduced(capi, m0, seq)
    ch, sim, last = m0.changed_mask(red)
    ch2, sim2, last2 = m0.changed_mask(red[3:], prev_small=last)
    sel = np.nonzero(ch2)[0]
    want = _trace(m0, m0.match_kept_frames(sel))
    assert ch.any() and not ch.all()
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    wc, wsim, wlast = mw.changed_mask(seq)
    assert np.array_equal(wc, ch) and wsim.tobytes() == sim.tobytes() and np.array_equal(wlast, last)
    wc2, wsim2, wlast2 = mw.changed_mask(seq[3:], prev_small=wlast)
    assert np.array_equal(wc2, ch2) and wsim2.tobytes() == sim2.tobytes() and np.array_equal(wlast2, last2)
    assert _trace(mw, mw.match_kept_frames(sel)) == want
    mw.close(); m0.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("pitched", [False, True])
def test_yuv420_twins(capi, deck, fmt, pitched):
    """Reduce comes after convert: the comparison side is the BGR call on the tap's reduction of the conversion tap's image."""
    import torch
    import yuv420_ref as ref
    pages, sets = deck
    frames, _ = sets["4k"]
    frames = frames[:4]
    n, h, w, _ = frames.shape
    L, fb = capi.yuv420_layout(fmt, w, h, pitch=-(-w // 256) * 256 + 256, row_align=16) if pitched else capi.yuv420_layout(fmt, w, h)
    yuv = ref.frames_to_yuv(frames, L, fb)
    mw, m0 = _matcher(capi, pages, WS), _matcher(capi, pages)
    bgr = np.stack([m0.yuv420_to_bgr(f, w, h, L) for f in yuv])
    red = _reduced(capi, m0, bgr)
    want = _trace(m0, m0.match_frames(red))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames_yuv420(yuv, w, h, L)) == want, "host"
    d = torch.from_numpy(yuv).cuda()
    assert _trace(mw, mw.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, yuv.shape[1])) == want, "device"
    v = mw.collect(mw.submit_yuv420_dev(d.data_ptr(), n, w, h, L, yuv.shape[1]))
    assert _trace(mw, v) == want, "submit / collect"
    seq, rseq = np.repeat(yuv[:2], 2, axis=0), np.repeat(red[:2], 2, axis=0)
    ch, sim, last = m0.changed_mask(rseq)
    wc, wsim, wlast = mw.changed_mask_yuv420(seq, w, h, L)
    assert np.array_equal(wc, ch) and wsim.tobytes() == sim.tobytes() and np.array_equal(wlast, last)
    sel = np.nonzero(ch)[0]
    assert mw.match_kept_frames(sel).tobytes() == m0.match_kept_frames(sel).tobytes()
    mw.close(); m0.close()


def test_group(capi, deck):
    """Two members on two devices where they exist, else one member."""
    pages, sets = deck
    frames, _ = sets["4k"]
    devs = capi.device_list()
    devs = devs[:2] if len(devs) >= 2 else devs[:1]
    m0 = _matcher(capi, pages)
    red = _reduced(capi, m0, frames)
    want = m0.match_frames(red)
    _paged(want)
    cands = [m0.last_candidates(i).tobytes() for i in range(len(red))]
    seq, rseq = np.repeat(frames[:4], 2, axis=0), np.repeat(red[:4], 2, axis=0)
    ch, sim, last = m0.changed_mask(rseq)
    sel = np.nonzero(ch)[0]
    want_kept = m0.match_kept_frames(sel)
    m0.close()
    g = capi.Group(capi.default_config(**CFG), devs)
    g.add_pages(list(pages))
    g.finalize()
    g.set_working_size(*WS)
    assert g.working_size == WS and g.member(0).working_size == WS
    assert g.match_frames(frames).tobytes() == want.tobytes()
    assert [g.last_candidates(i).tobytes() for i in range(len(frames))] == cands
    gc, gs, gl = g.changed_mask(seq)
    assert np.array_equal(gc, ch) and gs.tobytes() == sim.tobytes() and np.array_equal(gl, last)
    assert g.match_kept_frames(sel).tobytes() == want_kept.tobytes()
    g.set_working_size(0, 0)
    assert g.match_frames(red).tobytes() == want.tobytes()
    g.close()


def _mode_equal(capi, deck, key="4k", n=8, prepare=None, **kw):
    pages, sets = deck
    frames, _ = sets[key]
    frames = frames[:n]
    mw, m0 = _matcher(capi, pages, WS, **kw), _matcher(capi, pages, **kw)
    if prepare:
        prepare(mw); prepare(m0)
    want = _trace(m0, m0.match_frames(_reduced(capi, m0, frames)))
    got = _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == want
    mw.close(); m0.close()
    return got


@pytest.mark.parametrize("key", ["4k", "qhd"])
def test_mode_homography(capi, deck, key):
    _mode_equal(capi, deck, key, verify_model=1)


@pytest.mark.parametrize("key", ["4k", "qhd"])
def test_mode_ratio_test(capi, deck, key):
    _mode_equal(capi, deck, key, ratio_test=0.9)


@pytest.mark.parametrize("key", ["4k", "qhd"])
def test_mode_lsh(capi, deck, key):
    _mode_equal(capi, deck, key, matcher=1)


def test_mode_page_set(capi, deck):
    pages, sets = deck
    truth = sets["4k"][1]
    sel = sorted(set(int(t) for t in truth))                     # the pages the frames show (every frame keeps its page in the set)
    assert 1 <= len(sel) <= 6

    def prepare(m):
        m.use_page_set(m.create_page_set(sel))
    _mode_equal(capi, deck, "4k", prepare=prepare)


def test_mode_sift_and_a_4096_wide_source(capi, deck, synth):
    pages, sets = deck
    sift = (capi.sift_config(nfeatures=1000), 0.0)
    _mode_equal(capi, deck, "4k", n=4, sift=sift)
    wide, _ = _slides(synth, pages, 4, 4096, 2160)
    mw, m0 = _matcher(capi, pages, WS, sift=sift), _matcher(capi, pages, sift=sift)
    with pytest.raises(capi.SlideoError) as e:                   # refused without a working size: sides <= 4095
        m0.match_frames(wide)
    assert e.value.code == 5
    red = _reduced(capi, m0, wide)
    assert red.shape[1:3] == (1013, 1920)
    want = _trace(m0, m0.match_frames(red))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(wide)) == want
    mw.close(); m0.close()


def test_frames_that_fit_are_untouched(capi, deck, monkeypatch):
    """Under a working size, frames that fit give the unset matcher's results and unit sizes (the per-slot budget a refused
    submit reports); set then clear behaves the same."""
    import torch
    monkeypatch.setenv("SLIDEO_WS_GB", "0.6")
    pages, sets = deck
    m0 = _matcher(capi, pages)
    red = _reduced(capi, m0, sets["4k"][0])
    want = _trace(m0, m0.match_frames(red))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    d = torch.from_numpy(red).cuda()

    def budget(m):
        with pytest.raises(capi.SlideoError) as e:
            m.submit_dev(d.data_ptr(), 4096, 1920, 1080)
        assert e.value.code == 7
        return str(e.value)
    b0 = budget(m0)
    mw = _matcher(capi, pages, WS)
    assert _trace(mw, mw.match_frames(red)) == want
    assert _trace(mw, mw.match_frames_dev(d.data_ptr(), len(red), 1920, 1080)) == want
    assert budget(mw) == b0
    mw.set_working_size(4096, 4096)
    assert _trace(mw, mw.match_frames(red)) == want and budget(mw) == b0
    mw.set_working_size(1280, 720)
    assert _trace(mw, mw.match_frames(red)) != want
    mw.set_working_size(0, 0)
    assert mw.working_size == (0, 0)
    assert _trace(mw, mw.match_frames(red)) == want and budget(mw) == b0
    mw.close(); m0.close()


def test_errors(capi, deck):
    import torch
    pages, sets = deck
    frames = sets["4k"][0][:2]
    m = _matcher(capi, pages)

    def code(fn):
        with pytest.raises(capi.SlideoError) as e:
            fn()
        return e.value.code, str(e.value)
    for bad in ((0, 1080), (1920, 0), (-1, -1), (-1920, 1080)):
        assert code(lambda: m.set_working_size(*bad))[0] == 1, bad
    assert m.working_size == (0, 0)
    # a unit in flight
    d = torch.from_numpy(frames).cuda()
    t = m.submit_dev(d.data_ptr(), 2, 3840, 2160)
    assert code(lambda: m.set_working_size(*WS))[0] == 4
    m.collect(t)
    m.set_working_size(*WS)
    # a reduced size below small_area (120000): 320x180
    m.set_working_size(320, 180)
    c, msg = code(lambda: m.match_frames(frames))
    assert c == 5 and "320x180" in msg, msg
    c, msg = code(lambda: m.changed_mask(frames))
    assert c == 5 and "320x180" in msg, msg
    # kept frames end with a set
    m.set_working_size(*WS)
    m.changed_mask(frames)
    assert len(m.match_kept_frames([0])) == 1
    m.changed_mask(frames)
    m.set_working_size(*WS)
    assert code(lambda: m.match_kept_frames([0]))[0] == 4
    # the tap: no upscale, no copy
    img = frames[0]
    for dw, dh in ((3841, 2160), (3840, 2161), (3840, 2160), (0, 10), (10, 0)):
        assert code(lambda: m.reduce(img, dw, dh))[0] == 1, (dw, dh)
    assert m.reduce(img, 3840, 1080).shape == (1080, 3840, 3)
    m.close()
