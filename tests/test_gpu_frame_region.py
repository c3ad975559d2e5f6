"""Frame region (include/slideo_amd.h "Frame region"): the rectify tap (csrc/frame_region.hip.h) equals the numpy restatement
tests/frame_region_ref.py bit for bit and lies within the derived bound of the float64 definition; every frame call made under a
region returns, byte for byte, what the same call without one returns on the tap's output; the errors and refusals.

Inputs of the end-to-end tests: 6 synthetic pages of 2001x1125 and the first 8 frames of synth.frames at 2400x1350 that show a
slide, ORB-1000 and the default config otherwise; the region maps 1920x1080 onto the mildly keystoned quad QUAD, which covers most
of the frame.  (A stronger keystone — corners up to 210 pixels inside the frame — cuts into the slides the synthetic frames show and
left the restatement with 2 of 8 frames assigned in the default mode: the quad was made milder, as the premise demands.)  Every end-to-end test asserts that at least three quarters of the frames receive a page on the COMPARISON side (the
call without a region on the rectified images).  The CPU restatement alone meets that on these inputs — pyoracle.PageDB.match_frames
on frame_region_ref.rectify outputs of the very frames, pages assigned of frames (all equal to the synthetic truth):

    mode                      2400x1350 -> 1920x1080
    default                   8 / 8
    verify_model 1            8 / 8
    ratio_test 0.9            6 / 8      (the six assigned equal the truth)
    matcher 1                 8 / 8
    SIFT (ratio 0), 4 frames  4 / 4

(The page-set test selects the pages the frames show, the 4:2:0 tests read the converted images of the first four frames and the
masked test hides a corner strip: the restatement was not run on those; their comparison sides carry the same assertion on the
GPU.)

Under a region EVERY frame call of the matcher rectifies (a frame of another size is an error), so the four units in flight of the
submit / collect test all rectify: two BGR units and two NV12 units.
"""
import os

import numpy as np
import pytest

import frame_region_ref as R
from f64_checks import report

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
SRC = (2400, 1350)
OUT = (1920, 1080)
QUAD = [(30.5, 20.25), (2370.0, 12.5), (2385.75, 1338.0), (15.0, 1330.5)]
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
    return pages, _slides(synth, pages, 8, *SRC)


def _matcher(capi, pages, region=True, sift=None, **kw):
    m = capi.Matcher(capi.default_config(**dict(CFG, **kw)))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if region:
        m.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    return m


def _rect(m, frames):
    """The tap's output for frames [n, h, w, 3] under m's region."""
    return np.stack([m.rectify(f) for f in frames])


def _trace(m, v):
    """A call's verdict records and candidate traces as raw bytes."""
    return v.tobytes(), [m.last_candidates(i).tobytes() for i in range(len(v))]


def _paged(v):
    """The condition of every end-to-end test: three quarters of the comparison side's frames receive a page."""
    got = int((v["page_idx"] >= 0).sum())
    assert 4 * got >= 3 * len(v), (got, len(v))
    return got


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- the tap ---------------------------------------------------------------------------------------------------------------------

def _quad_map(quad, ow, oh):
    """The map of a quad by numpy's solver (the tap tests need a map, not the library's)."""
    A, b = [], []
    for (u, v), (x, y) in zip([(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)], quad):
        A.append([u, v, 1, 0, 0, 0, -x * u, -x * v]); b.append(x)
        A.append([0, 0, 0, u, v, 1, -y * u, -y * v]); b.append(y)
    return np.append(np.linalg.solve(np.array(A, float), np.array(b, float)), 1.0)


# (name, source w x h, stride or None, M, out w x h) and what each can break
TAP_SHAPES = [
    # the quad partly outside the source: the replicate clamp on all four sides
    ("outside", 97, 61, None, _quad_map([(-6.3, -4.2), (101.5, 3.0), (99.0, 66.7), (-3.5, 58.1)], 64, 40), 64, 40),
    # out width not a multiple of 4 (byte stores), a pitched source, x crossing bw0 = 64 twice
    ("pitched", 200, 120, 607, _quad_map([(10.2, 8.1), (190.5, 3.3), (195.0, 115.7), (4.5, 110.1)], 133, 77), 133, 77),
    # out_h < 16: bw0 = 1024 / 5 = 204, clipped to 200
    ("low", 300, 40, None, _quad_map([(5.5, 3.2), (290.1, 1.0), (295.0, 36.7), (2.5, 38.1)], 200, 5), 200, 5),
    ("upscale", 64, 64, None, _quad_map([(1.5, 2.2), (61.1, 0.5), (63.0, 62.7), (0.5, 60.1)], 128, 128), 128, 128),
    # the affine instance: a rotation by 90 degrees, and a general affine map with M8 != 1
    ("rot90", 80, 120, None, [0, 1, 0, -1, 0, 119, 0, 0, 1], 120, 80),
    ("affine", 80, 120, None, [0.7, 0.2, 3.3, -0.1, 0.9, 5.5, 0, 0, 2.0], 90, 70),
    # the integer-translation instance: the dword copy, and the byte copy that runs over the border
    ("crop", 200, 120, None, [1, 0, 20, 0, 1, 8, 0, 0, 1], 100, 64),
    ("crop-border", 200, 120, 601, [1, 0, -3, 0, 1, -2, 0, 0, 1], 101, 130),
    ("1wide", 1, 50, None, _quad_map([(-1, 0), (1.5, 2), (2, 48), (-1, 49)], 16, 40), 16, 40),
    ("1high", 50, 1, None, _quad_map([(0, -1), (48.5, -2), (49, 2), (1, 1)], 40, 16), 40, 16),
    # more than one block along x and y at the end-to-end size's map
    ("keystone", 600, 338, None, _quad_map([(53.1, 35.0), (547.5, 24.1), (562.9, 315.5), (40.0, 303.9)], 480, 270), 480, 270),
]


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(capi.default_config(**CFG))
    yield m
    m.close()


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: s[0])
def test_tap_equals_the_restatement(tap, shape):
    name, w, h, stride, M, ow, oh = shape
    stride = stride or w * 3
    rng = np.random.default_rng(w * 5 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)          # (the pitch bytes are noise: they must not be read)
    buf[:, :w * 3] = img.reshape(h, w * 3)
    tap.set_frame_region(w, h, M, ow, oh)
    reg = tap.frame_region
    assert reg[0] == w and reg[1] == h and reg[3] == ow and reg[4] == oh and reg[2].reshape(9).tolist() == [float(v) for v in M]
    got = tap.rectify_pitched(buf, w, h, stride)
    want = R.rectify(img, M, ow, oh)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4])
    if name == "crop":
        assert np.array_equal(got, img[8:8 + 64, 20:20 + 100])
    tap.clear_frame_region()
    assert tap.frame_region is None


@pytest.mark.parametrize("name", ["pitched", "upscale", "keystone", "outside"])
def test_tap_against_the_float64_definition(tap, synth, name):
    """|R - bilinear_f64(I, exact coordinate)| <= 0.5 + (Dx + Dy) / 64 + 1e-6: the coordinate is quantised to 1/32 (at most 1/64
    off along x and along y), bilinear interpolation is Lipschitz along x (y) with the largest step between horizontally
    (vertically) adjacent pixels around the coordinate — Dx (Dy), taken within 2 pixels of it — and the blend with the table's exact
    integer weights is rounded once (0.5).  Content: a synthetic slide frame (smooth and sharp regions; noise would make the bound
    vacuous)."""
    _, w, h, _, M, ow, oh = next(s for s in TAP_SHAPES if s[0] == name)
    img = synth.frames(synth.pages(2, 800, 450), 1, w, h, first=3)[0][0]
    tap.set_frame_region(w, h, M, ow, oh)
    got = tap.rectify(img).astype(np.float64)
    tap.clear_frame_region()
    u, v = R.exact_coords(M, ow, oh)
    ideal = R.bilinear_f64(img, u, v)
    Dx, Dy = R.local_steps(img, u, v)
    bound = 0.5 + (Dx + Dy)[:, :, None] / 64.0 + 1e-6
    dev = np.abs(got - ideal)
    report("rectify", shape=name, max_dev=float(dev.max()), max_bound=float(bound.max()), median_bound=float(np.median(bound)),
           worst_margin=float((bound - dev).min()))
    assert (dev <= bound).all(), (float(dev.max()), np.argwhere(dev > bound)[:4])


# ---- every frame path ------------------------------------------------------------------------------------------------------------

def test_host_and_device_calls(capi, deck):
    import torch
    pages, (frames, truth) = deck
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    rect = _rect(mw, frames)
    assert rect.shape == (n, OUT[1], OUT[0], 3)
    assert np.array_equal(rect[0], R.rectify(frames[0], capi.frame_region_from_quad(QUAD, *OUT), *OUT)), "the tap at the end-to-end size"
    want = _trace(m0, m0.match_frames(rect))
    v0 = np.frombuffer(want[0], capi.VERDICT_DTYPE)
    _paged(v0)
    assert (v0["page_idx"] == truth).mean() >= 0.75
    assert _trace(mw, mw.match_frames(frames)) == want, "pageable host frames"
    pin = torch.from_numpy(frames).pin_memory()
    assert _trace(mw, mw.match_frames(pin.numpy())) == want, "pinned host frames"
    d = torch.from_numpy(frames).cuda()
    assert _trace(mw, mw.match_frames_dev(d.data_ptr(), n, w, h)) == want, "device frames"
    stride = w * 3 + 61                                            # rows at every byte alignment
    dp = torch.zeros((n, h + 1, stride), dtype=torch.uint8, device="cuda")
    dp[:, :h, :w * 3] = d.reshape(n, h, w * 3)
    torch.cuda.synchronize()
    assert _trace(mw, mw.match_frames_dev(dp.data_ptr(), n, w, h, stride, stride * (h + 1))) == want, "pitched device frames"
    # NULL clears the region: the results of a matcher that never had one
    mw.clear_frame_region()
    assert mw.frame_region is None
    assert _trace(mw, mw.match_frames(rect)) == want
    mw.close(); m0.close()


def test_submit_collect_four_units_in_flight(capi, deck):
    import torch
    import yuv420_ref as ref
    pages, (frames, _) = deck
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = ref.frames_to_yuv(frames[4:], L, fb)
    bgr = np.stack([m0.yuv420_to_bgr(f, w, h, L) for f in yuv])
    rect = np.concatenate([_rect(mw, frames[:4]), _rect(mw, bgr)])
    assert mw.max_in_flight() >= 4
    d0 = [torch.from_numpy(np.ascontiguousarray(rect[i:i + 2])).cuda() for i in range(0, 8, 2)]
    t0 = [m0.submit_dev(d.data_ptr(), 2, OUT[0], OUT[1]) for d in d0]
    want = _trace(m0, np.concatenate([m0.collect(t) for t in t0]))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    db = [torch.from_numpy(np.ascontiguousarray(frames[i:i + 2])).cuda() for i in (0, 2)]
    dy = [torch.from_numpy(np.ascontiguousarray(yuv[i:i + 2])).cuda() for i in (0, 2)]
    tickets = [mw.submit_dev(d.data_ptr(), 2, w, h) for d in db] + [mw.submit_yuv420_dev(d.data_ptr(), 2, w, h, L, fb) for d in dy]
    # a region on a busy matcher
    assert _code(capi, lambda: mw.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1]))[0] == 4
    assert _code(capi, mw.clear_frame_region)[0] == 4
    got = _trace(mw, np.concatenate([mw.collect(t) for t in tickets]))
    assert got == want
    mw.close(); m0.close()


def test_changed_mask_and_kept_frames(capi, deck):
    pages, (frames, _) = deck
    seq = np.repeat(frames[:4], 2, axis=0)                       # every frame twice: unchanged and changed flags both occur
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    rect = np.repeat(_rect(mw, frames[:4]), 2, axis=0)
    ch, sim, last = m0.changed_mask(rect)
    ch2, sim2, last2 = m0.changed_mask(rect[3:], prev_small=last)
    sel = np.nonzero(ch2)[0]
    want = _trace(m0, m0.match_kept_frames(sel))
    assert ch.any() and not ch.all()
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    wc, wsim, wlast = mw.changed_mask(seq)
    assert np.array_equal(wc, ch) and wsim.tobytes() == sim.tobytes() and np.array_equal(wlast, last)
    wc2, wsim2, wlast2 = mw.changed_mask(seq[3:], prev_small=wlast)
    assert np.array_equal(wc2, ch2) and wsim2.tobytes() == sim2.tobytes() and np.array_equal(wlast2, last2)
    assert _trace(mw, mw.match_kept_frames(sel)) == want
    # kept frames end with a set
    mw.changed_mask(seq[:2])
    mw.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    assert _code(capi, lambda: mw.match_kept_frames([0]))[0] == 4
    mw.close(); m0.close()


@pytest.mark.parametrize("direct", [0.0, 0.9])
def test_gated_calls(capi, deck, direct):
    import torch
    pages, (frames, _) = deck
    seq = np.repeat(frames[:6], 2, axis=0)[1:]                   # 11 frames; the first is primed from the frame before it
    n, h, w, _ = seq.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    rect = np.repeat(_rect(mw, frames[:6]), 2, axis=0)
    rseq = rect[1:]
    if direct:
        mw.set_direct_similarity(direct); m0.set_direct_similarity(direct)

    def gated(m, out):
        ch, sim, v = out
        return ch.tobytes(), sim.tobytes(), v.tobytes(), [m.last_candidates(i).tobytes() for i in range(int(ch.sum()) - int(((v["page_idx"] >= 0) & (v["inliers"] == 0) & ch).sum()))]
    # host, primed from a host frame
    m0.gate_reset_from_frame(rect[0]); mw.gate_reset_from_frame(frames[0])
    want = gated(m0, m0.match_changed_frames(rseq))
    ch = np.frombuffer(want[0], np.uint8).astype(bool)
    assert ch.any() and not ch.all()
    _paged(np.frombuffer(want[2], capi.VERDICT_DTYPE)[ch])
    assert gated(mw, mw.match_changed_frames(seq)) == want, "host"
    assert np.array_equal(mw.gate_last_small(), m0.gate_last_small())
    # device, primed from a device frame; then the submit / collect form continuing the state
    d0, dw = torch.from_numpy(rect).cuda(), torch.from_numpy(np.concatenate([frames[:1], seq])).cuda()
    fb0, fbw = OUT[0] * OUT[1] * 3, w * h * 3
    m0.gate_reset_from_frame_dev(d0.data_ptr(), OUT[0], OUT[1]); mw.gate_reset_from_frame_dev(dw.data_ptr(), w, h)
    assert gated(mw, mw.match_changed_frames_dev(dw.data_ptr() + fbw, n, w, h)) == gated(m0, m0.match_changed_frames_dev(d0.data_ptr() + fb0, n, OUT[0], OUT[1])) == want
    a0 = m0.collect_changed(m0.submit_changed_dev(d0.data_ptr() + fb0, 5, OUT[0], OUT[1]))
    aw = mw.collect_changed(mw.submit_changed_dev(dw.data_ptr() + fbw, 5, w, h))
    assert gated(mw, aw) == gated(m0, a0)
    # a set resets the gate state to "none": the next gated frame is changed
    mw.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    assert _code(capi, mw.gate_last_small)[0] == 4
    mw.close(); m0.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("pitched", [False, True])
def test_yuv420_twins(capi, deck, fmt, pitched):
    """Rectify comes after convert: the comparison side is the BGR call on the tap's output for the conversion tap's image."""
    import torch
    import yuv420_ref as ref
    pages, (frames, _) = deck
    frames = frames[:4]
    n, h, w, _ = frames.shape
    L, fb = capi.yuv420_layout(fmt, w, h, pitch=-(-w // 256) * 256 + 256, row_align=16) if pitched else capi.yuv420_layout(fmt, w, h)
    yuv = ref.frames_to_yuv(frames, L, fb)
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    bgr = np.stack([m0.yuv420_to_bgr(f, w, h, L) for f in yuv])
    rect = _rect(mw, bgr)
    want = _trace(m0, m0.match_frames(rect))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames_yuv420(yuv, w, h, L)) == want, "host"
    d = torch.from_numpy(yuv).cuda()
    assert _trace(mw, mw.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, yuv.shape[1])) == want, "device"
    seq, rseq = np.repeat(yuv[:2], 2, axis=0), np.repeat(rect[:2], 2, axis=0)
    ch, sim, last = m0.changed_mask(rseq)
    wc, wsim, wlast = mw.changed_mask_yuv420(seq, w, h, L)
    assert np.array_equal(wc, ch) and wsim.tobytes() == sim.tobytes() and np.array_equal(wlast, last)
    g0, gw = m0.match_changed_frames(rseq), mw.match_changed_frames_yuv420(seq, w, h, L)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(g0, gw)), "gated"
    mw.close(); m0.close()


def test_group(capi, deck):
    """Two members on two devices where they exist, else one member."""
    pages, (frames, _) = deck
    devs = capi.device_list()
    devs = devs[:2] if len(devs) >= 2 else devs[:1]
    g = capi.Group(capi.default_config(**CFG), devs)
    g.add_pages(list(pages))
    g.finalize()
    g.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    assert g.frame_region[3:] == OUT and g.member(0).frame_region[:2] == SRC
    rect = np.stack([g.rectify(f) for f in frames])
    m0 = _matcher(capi, pages, region=False)
    want = m0.match_frames(rect)
    _paged(want)
    cands = [m0.last_candidates(i).tobytes() for i in range(len(rect))]
    seq, rseq = np.repeat(frames[:4], 2, axis=0), np.repeat(rect[:4], 2, axis=0)
    ch, sim, last = m0.changed_mask(rseq)
    sel = np.nonzero(ch)[0]
    want_kept = m0.match_kept_frames(sel)
    m0.gate_reset()
    want_gated = m0.match_changed_frames(rseq)
    m0.close()
    assert g.match_frames(frames).tobytes() == want.tobytes()
    assert [g.last_candidates(i).tobytes() for i in range(len(frames))] == cands
    gc, gs, gl = g.changed_mask(seq)
    assert np.array_equal(gc, ch) and gs.tobytes() == sim.tobytes() and np.array_equal(gl, last)
    assert g.match_kept_frames(sel).tobytes() == want_kept.tobytes()
    got_gated = g.match_changed_frames(seq)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got_gated, want_gated))
    g.clear_frame_region()
    assert g.frame_region is None
    assert g.match_frames(rect).tobytes() == want.tobytes()
    g.close()


def test_frame_mask_of_the_output_size(capi, deck):
    pages, (frames, _) = deck
    mask = np.full((OUT[1], OUT[0]), 255, np.uint8)
    mask[-300:, -480:] = 0                                        # a speaker inset in the rectified image's corner
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, region=False)
    rect = _rect(mw, frames)
    plain = _trace(m0, m0.match_frames(rect))
    mw.set_frame_mask(mask); m0.set_frame_mask(mask)
    want = _trace(m0, m0.match_frames(rect))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert want != plain
    assert _trace(mw, mw.match_frames(frames)) == want
    # a mask of the SOURCE size is an error under the region
    mw.set_frame_mask(np.full((SRC[1], SRC[0]), 255, np.uint8))
    assert _code(capi, lambda: mw.match_frames(frames))[0] == 1
    mw.close(); m0.close()


def _mode_equal(capi, deck, n=8, prepare=None, **kw):
    pages, (frames, _) = deck
    frames = frames[:n]
    mw, m0 = _matcher(capi, pages, **kw), _matcher(capi, pages, region=False, **kw)
    if prepare:
        prepare(mw); prepare(m0)
    want = _trace(m0, m0.match_frames(_rect(mw, frames)))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == want
    mw.close(); m0.close()


def test_mode_homography(capi, deck):
    _mode_equal(capi, deck, verify_model=1)


def test_mode_ratio_test(capi, deck):
    _mode_equal(capi, deck, ratio_test=0.9)


def test_mode_lsh(capi, deck):
    _mode_equal(capi, deck, matcher=1)


def test_mode_page_set(capi, deck):
    sel = sorted(set(int(t) for t in deck[1][1]))                 # the pages the frames show (every frame keeps its page in the set)
    assert 1 <= len(sel) <= 6
    _mode_equal(capi, deck, prepare=lambda m: m.use_page_set(m.create_page_set(sel)))


def test_mode_sift(capi, deck):
    _mode_equal(capi, deck, n=4, sift=(capi.sift_config(nfeatures=1000), 0.0))


# ---- errors ----------------------------------------------------------------------------------------------------------------------

def test_errors_and_refusals(capi, deck):
    pages, (frames, _) = deck
    frames = frames[:2]
    m = _matcher(capi, pages, region=False)
    I = [1.0, 0, 0, 0, 1, 0, 0, 0, 1]

    def set_(sw, sh, M, ow, oh):
        return _code(capi, lambda: m.set_frame_region(sw, sh, M, ow, oh))
    # set-time refusals, the rule named
    for bad in (float("nan"), float("inf")):
        c, msg = set_(640, 360, [1.0, 0, bad, 0, 1, 0, 0, 0, 1], 320, 180)
        assert c == 1 and "finite" in msg, msg
    for M in ([1.0, 0, 0, 0, 1, 0, 0, 0, 0],                      # W == 0 everywhere
              [1.0, 0, 0, 0, 1, 0, -1.0 / 100, 0, 1],             # W changes sign along x (zero at x = 100 < 319)
              [1.0, 0, 0, 0, 1, 0, 0, -1.0 / 128, 1]):            # W is exactly zero at the bottom corners (y = 128)
        c, msg = set_(640, 360, M, 320, 129)
        assert c == 1 and "W" in msg and "sign" in msg, msg
    for ow, oh in ((0, 180), (320, 0), (4097, 180), (320, 4097), (-1, -1)):
        c, msg = set_(640, 360, I, ow, oh)
        assert c == 1 and "output size" in msg, msg
    for sw, sh in ((0, 360), (640, 0), (4097, 360), (640, 4097)):
        c, msg = set_(sw, sh, I, 320, 180)
        assert c == 1 and "source size" in msg, msg
    assert m.frame_region is None
    # the wrong source size names both sizes; nothing is silently left unrectified
    m.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    small = np.ascontiguousarray(frames[:, :1080, :1920])
    for fn in (lambda: m.match_frames(small), lambda: m.changed_mask(small), lambda: m.match_changed_frames(small),
               lambda: m.gate_reset_from_frame(small[0]), lambda: m.rectify(small[0])):
        c, msg = _code(capi, fn)
        assert c == 1 and "1920x1080" in msg and "2400x1350" in msg, msg
    # the limits apply to the output size: below small_area (120000)
    m.set_frame_region(SRC[0], SRC[1], QUAD, 320, 180)
    c, msg = _code(capi, lambda: m.match_frames(frames))
    assert c == 5 and "320x180" in msg, msg
    assert m.rectify(frames[0]).shape == (180, 320, 3)           # (the tap applies no such limit)
    # the working size, in both orders; the source is exempt from it, the output must fit it
    m.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    c, msg = _code(capi, lambda: m.set_working_size(1280, 720))
    assert c == 5 and "1280x720" in msg and "1920x1080" in msg, msg
    assert m.working_size == (0, 0)
    m.set_working_size(1920, 1080)                                # fits: the 2400x1350 source is not reduced
    want = m.match_frames(frames).tobytes()
    m.set_working_size(0, 0)
    assert m.match_frames(frames).tobytes() == want
    m.clear_frame_region()
    m.set_working_size(1280, 720)
    c, msg = set_(SRC[0], SRC[1], capi.frame_region_from_quad(QUAD, *OUT), OUT[0], OUT[1])
    assert c == 5 and "1280x720" in msg and "1920x1080" in msg, msg
    assert m.frame_region is None
    m.set_frame_region(SRC[0], SRC[1], QUAD, 1280, 720)
    assert m.frame_region[3:] == (1280, 720)
    # the tap without a region
    m.clear_frame_region()
    assert _code(capi, lambda: m.rectify(frames[0]))[0] == 4
    m.close()
