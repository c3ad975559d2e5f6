"""Frame lens (include/slideo_amd.h "Frame lens") on the GPU: the tap (csrc/frame_lens.hip.h) equals the numpy restatement
tests/frame_lens_ref.py bit for bit and lies within the derived bound of the float64 definition; every call that stages frames
returns under a lens, byte for byte, what the same call under the default returns on the tap's images; the errors and refusals; the
off value.

Inputs of the end-to-end tests: 6 synthetic pages of 1600x900 and the first 8 frames of synth.frames at 960x540 that show a slide,
bent by the lens k1 = -0.08 at f = half the diagonal (frame_lens_ref.bend: the forward model, nothing of the code under test), ORB-1000
and the default config otherwise.  Every end-to-end test asserts that at least three quarters of the comparison side's frames
receive a page.  The CPU restatement alone meets that on these inputs — pyoracle.PageDB.match_frames on frame_lens_ref.undistort
outputs of the very frames, pages assigned of frames (right: equal to the synthetic truth):

    mode                              assigned   right
    default                           8 / 8      8
    lens + region (QUAD -> 960x540)   8 / 8      5
    verify_model 1                    8 / 8      7
    ratio_test 0.97                   6 / 8      6      (0.9 assigns 4 of 8, 0.95 5 of 8: the ratio was raised, as the premise demands)
    matcher 1                         8 / 8      8
    SIFT (ratio 0), 4 frames          4 / 4      4
    the bent frames, nothing set      8 / 8      4

(The page-set test selects the pages the frames show, the YUV and RGBA tests read the converted images of the first four frames, the
masked and the shading / levels tests change the picture: the restatement was not run on those; their comparison sides carry the
same assertion on the GPU.)"""
import numpy as np
import pytest

import frame_lens_ref as FL
import frame_region_ref as R
import levels_ref as LR
import shading_ref as SR
from f64_checks import report
from test_frame_lens_abi import TAP_SHAPES, quad_map, tap_input

pytestmark = pytest.mark.gpu

SRC = (960, 540)
LENS = SRC + FL.defaults(*SRC) + (-0.08, 0.0)           # what set_frame_lens takes
QUAD = [(12.5, 8.25), (948.0, 5.5), (952.75, 533.0), (6.0, 531.5)]      # in IDEAL coordinates
OUT = (960, 540)
CFG = dict(nfeatures=1000)


@pytest.fixture(scope="module")
def deck(synth):
    pages = synth.pages(6, 1600, 900, threads=8)
    fr, truth, _ = synth.frames(pages, 16, *SRC, threads=8)
    keep = np.nonzero(truth >= 0)[0][:8]
    assert len(keep) == 8
    return pages, (FL.bend(fr[keep], LENS[2:]), truth[keep])


def _matcher(capi, pages, lens=True, region=False, sift=None, **kw):
    m = capi.Matcher(capi.default_config(**dict(CFG, **kw)))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if region:
        m.set_frame_region(SRC[0], SRC[1], QUAD, OUT[0], OUT[1])
    if lens:
        m.set_frame_lens(*LENS)
    return m


def _und(m, frames):
    """The tap's output for frames [n, h, w, 3] under m's lens (and region)."""
    return np.stack([m.undistort(f) for f in frames])


def _trace(m, v):
    """A call's verdict records and candidate traces as raw bytes."""
    return v.tobytes(), [m.last_candidates(i).tobytes() for i in range(len(v))]


def _paged(v):
    """The condition of every end-to-end test: three quarters of the comparison side's frames receive a page."""
    got = int((v["page_idx"] >= 0).sum())
    assert 4 * got >= 3 * len(v), (got, len(v))
    return got


def _same3(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- the tap ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(capi.default_config(**CFG))
    yield m
    m.close()


def _set(tap, shape):
    _, w, h, _, M, out, lens = shape
    tap.clear_frame_lens(); tap.clear_frame_region()
    if M is not None:
        tap.set_frame_region(w, h, M, out[0], out[1])
    tap.set_frame_lens(w, h, *lens)


@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: s[0])
def test_tap_equals_the_restatement(tap, shape):
    name, w, h, _, M, out, lens = shape
    img, buf, stride = tap_input(shape)                              # (the pitch bytes are noise: they must not be read)
    _set(tap, shape)
    assert tap.frame_lens == (w, h) + tuple(float(v) for v in lens)
    got = tap.undistort_pitched(buf, w, h, stride)
    want = FL.undistort(img, lens, M, *(out or (None, None)))
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, int((got != want).sum()), np.argwhere(got != want)[:4])
    if M is not None:                                                # slideo_rectify_bgr8 stays the tap of the region alone
        assert np.array_equal(tap.rectify_pitched(buf, w, h, stride), R.rectify(img, M, *out))
    tap.clear_frame_lens(); tap.clear_frame_region()
    assert tap.frame_lens is None


@pytest.mark.parametrize("name", ["barrel", "region", "blocks"])
def test_tap_against_the_float64_definition(tap, synth, name):
    """|U - bilinear_f64(I, exact coordinate)| <= 0.5 + (Dx + Dy) / 64 + 1e-6: the coordinate is quantised to 1/32 (at most 1/64 off
    along x and along y), bilinear interpolation is Lipschitz along x (y) with the largest step between horizontally (vertically)
    adjacent pixels around the coordinate — Dx (Dy), taken within 2 pixels of it — and the blend with the table's exact integer
    weights is rounded once (0.5).  Content: a synthetic slide frame (smooth and sharp regions; noise would make the bound vacuous)."""
    shape = next(s for s in TAP_SHAPES if s[0] == name)
    _, w, h, _, M, out, lens = shape
    ow, oh = out or (w, h)
    img = synth.frames(synth.pages(2, 800, 450), 1, w, h, first=3)[0][0]
    _set(tap, shape)
    got = tap.undistort(img).astype(np.float64)
    tap.clear_frame_lens(); tap.clear_frame_region()
    u, v = FL.exact_coords(lens, M, ow, oh)
    ideal = R.bilinear_f64(img, u, v)
    Dx, Dy = R.local_steps(img, u, v)
    bound = 0.5 + (Dx + Dy)[:, :, None] / 64.0 + 1e-6
    dev = np.abs(got - ideal)
    report("undistort", shape=name, max_dev=float(dev.max()), max_bound=float(bound.max()), median_bound=float(np.median(bound)),
           worst_margin=float((bound - dev).min()))
    assert (dev <= bound).all(), (float(dev.max()), np.argwhere(dev > bound)[:4])


# ---- every frame path ------------------------------------------------------------------------------------------------------------

def test_host_and_device_calls(capi, deck):
    import torch
    pages, (frames, truth) = deck
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, lens=False)
    und = _und(mw, frames)
    assert und.shape == frames.shape
    assert np.array_equal(und[0], FL.undistort(frames[0], LENS[2:])), "the tap at the end-to-end size"
    want = _trace(m0, m0.match_frames(und))
    v0 = np.frombuffer(want[0], capi.VERDICT_DTYPE)
    _paged(v0)
    assert (v0["page_idx"] == truth).mean() >= 0.75
    assert _trace(mw, mw.match_frames(frames)) == want, "pageable host frames"
    pin = torch.from_numpy(frames).pin_memory()
    assert _trace(mw, mw.match_frames(pin.numpy())) == want, "pinned host frames"
    d = torch.from_numpy(frames).cuda()
    keep = d.clone()
    assert _trace(mw, mw.match_frames_dev(d.data_ptr(), n, w, h)) == want, "device frames"
    stride = w * 3 + 61                                            # rows at every byte alignment
    dp = torch.zeros((n, h + 1, stride), dtype=torch.uint8, device="cuda")
    dp[:, :h, :w * 3] = d.reshape(n, h, w * 3)
    torch.cuda.synchronize()
    assert _trace(mw, mw.match_frames_dev(dp.data_ptr(), n, w, h, stride, stride * (h + 1))) == want, "pitched device frames"
    assert torch.equal(d, keep), "a device frame is never written"
    # a frame list: separate host frames
    assert _trace(mw, mw.match_frames([f for f in frames])) == want, "a frame list"
    # the observe calls see the undistorted frames
    for x, f in ((m0, und), (mw, frames)):
        x.activity_begin(12); x.observe_frames(f[:4])
    a, b = mw.activity_counts(), m0.activity_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    mw.activity_end(); m0.activity_end()
    # off clears the lens: the results of a matcher that never had one
    mw.clear_frame_lens()
    assert mw.frame_lens is None
    assert _trace(mw, mw.match_frames(und)) == want
    mw.close(); m0.close()


def test_submit_collect_four_units_in_flight(capi, deck):
    import torch
    import yuv420_ref as ref
    pages, (frames, _) = deck
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, lens=False)
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = ref.frames_to_yuv(frames[4:], L, fb)
    bgr = np.stack([m0.yuv420_to_bgr(f, w, h, L) for f in yuv])
    und = np.concatenate([_und(mw, frames[:4]), _und(mw, bgr)])
    assert mw.max_in_flight() >= 4
    d0 = [torch.from_numpy(np.ascontiguousarray(und[i:i + 2])).cuda() for i in range(0, 8, 2)]
    t0 = [m0.submit_dev(d.data_ptr(), 2, w, h) for d in d0]
    want = _trace(m0, np.concatenate([m0.collect(t) for t in t0]))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    db = [torch.from_numpy(np.ascontiguousarray(frames[i:i + 2])).cuda() for i in (0, 2)]
    dy = [torch.from_numpy(np.ascontiguousarray(yuv[i:i + 2])).cuda() for i in (0, 2)]
    tickets = [mw.submit_dev(d.data_ptr(), 2, w, h) for d in db] + [mw.submit_yuv420_dev(d.data_ptr(), 2, w, h, L, fb) for d in dy]
    # a lens on a busy matcher: a state error, and the lens stays
    assert _code(capi, lambda: mw.set_frame_lens(*LENS))[0] == 4
    assert _code(capi, mw.clear_frame_lens)[0] == 4
    assert mw.frame_lens == LENS
    got = _trace(mw, np.concatenate([mw.collect(t) for t in tickets]))
    assert got == want
    mw.close(); m0.close()


def test_changed_mask_and_kept_frames(capi, deck):
    pages, (frames, _) = deck
    seq = np.repeat(frames[:4], 2, axis=0)                       # every frame twice: unchanged and changed flags both occur
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, lens=False)
    und = np.repeat(_und(mw, frames[:4]), 2, axis=0)
    ch, sim, last = m0.changed_mask(und)
    sel = np.nonzero(ch)[0]
    want = _trace(m0, m0.match_kept_frames(sel))
    assert ch.any() and not ch.all()
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    wc, wsim, wlast = mw.changed_mask(seq)
    assert np.array_equal(wc, ch) and wsim.tobytes() == sim.tobytes() and np.array_equal(wlast, last)
    assert _trace(mw, mw.match_kept_frames(sel)) == want
    # kept frames end with a set; so does the gate state and an open match session
    mw.gate_reset_from_frame(frames[0])
    assert mw.gate_last_small().ndim == 3
    mw.placement_begin(32, 8, 6.0)
    mw.changed_mask(seq[:2])
    assert len(mw.match_kept_frames([0])) == 1
    mw.changed_mask(seq[:2])
    mw.set_frame_lens(*LENS)
    assert _code(capi, lambda: mw.match_kept_frames([0]))[0] == 4
    assert _code(capi, mw.gate_last_small)[0] == 4
    assert _code(capi, mw.placement_info)[0] == 4
    mw.close(); m0.close()


@pytest.mark.parametrize("direct", [0.0, 0.9])
def test_gated_calls(capi, deck, direct):
    import torch
    pages, (frames, _) = deck
    seq = np.repeat(frames[:6], 2, axis=0)[1:]                   # 11 frames; the first is primed from the frame before it
    n, h, w, _ = seq.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, lens=False)
    und = np.repeat(_und(mw, frames[:6]), 2, axis=0)
    useq = und[1:]
    if direct:
        mw.set_direct_similarity(direct); m0.set_direct_similarity(direct)
    m0.gate_reset_from_frame(und[0]); mw.gate_reset_from_frame(frames[0])
    want = m0.match_changed_frames(useq)
    ch = want[0].astype(bool)
    assert ch.any() and not ch.all()
    _paged(want[2][ch])
    assert _same3(mw.match_changed_frames(seq), want), "host"
    assert np.array_equal(mw.gate_last_small(), m0.gate_last_small())
    d0, dw = torch.from_numpy(und).cuda(), torch.from_numpy(np.concatenate([frames[:1], seq])).cuda()
    fb = w * h * 3
    m0.gate_reset_from_frame_dev(d0.data_ptr(), w, h); mw.gate_reset_from_frame_dev(dw.data_ptr(), w, h)
    assert _same3(mw.match_changed_frames_dev(dw.data_ptr() + fb, n, w, h), m0.match_changed_frames_dev(d0.data_ptr() + fb, n, w, h))
    a0 = m0.collect_changed(m0.submit_changed_dev(d0.data_ptr() + fb, 5, w, h))
    aw = mw.collect_changed(mw.submit_changed_dev(dw.data_ptr() + fb, 5, w, h))
    assert _same3(aw, a0)
    mw.close(); m0.close()


def test_yuv_twins_and_a_pixel_format(capi, deck):
    """The lens comes after the conversion: the comparison side is the BGR call on the tap's output for the conversion tap's image."""
    import torch
    import yuv420_ref as ref
    import yuv_desc_ref as dref
    pages, (frames, _) = deck
    frames = frames[:4]
    n, h, w, _ = frames.shape
    mw, m0 = _matcher(capi, pages), _matcher(capi, pages, lens=False)
    # NV12
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = ref.frames_to_yuv(frames, L, fb)
    und = _und(mw, np.stack([m0.yuv420_to_bgr(f, w, h, L) for f in yuv]))
    want = _trace(m0, m0.match_frames(und))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames_yuv420(yuv, w, h, L)) == want, "NV12 host"
    d = torch.from_numpy(yuv).cuda()
    assert _trace(mw, mw.match_frames_yuv420_dev(d.data_ptr(), n, w, h, L, yuv.shape[1])) == want, "NV12 device"
    # P010 under BT.709 limited
    desc = (dref.BT709, dref.LIMITED, dref.D10_MSB)
    for x in (mw, m0):
        x.set_yuv_description("bt709", "limited", "10_msb")
    L2, fb2 = capi.yuv420_layout("nv12", w, h, bytes_per_sample=2)
    p010 = dref.frames_to_yuv(frames, L2, fb2, desc)
    und = _und(mw, np.stack([m0.yuv420_to_bgr(f, w, h, L2) for f in p010]))
    want = _trace(m0, m0.match_frames(und))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames_yuv420(p010, w, h, L2)) == want, "P010 host"
    # RGBA through the BGR door
    und = _und(mw, frames)
    want = _trace(m0, m0.match_frames(und))
    mw.set_pixel_format("rgba")
    rgba = np.concatenate([frames[:, :, :, ::-1], np.full((n, h, w, 1), 99, np.uint8)], axis=3)
    assert _trace(mw, mw.match_frames(rgba)) == want, "RGBA"
    mw.close(); m0.close()


def test_group_of_two_members(capi, deck):
    pages, (frames, _) = deck
    g = capi.Group(capi.default_config(**CFG), [0, 0])
    g.add_pages(list(pages))
    g.finalize()
    g.set_frame_lens(*LENS)
    assert g.frame_lens == LENS and g.member(1).frame_lens == LENS
    und = np.stack([g.undistort(f) for f in frames])
    m0 = _matcher(capi, pages, lens=False)
    want = m0.match_frames(und)
    _paged(want)
    cands = [m0.last_candidates(i).tobytes() for i in range(len(und))]
    seq, useq = np.repeat(frames[:4], 2, axis=0), np.repeat(und[:4], 2, axis=0)
    ch, sim, last = m0.changed_mask(useq)
    sel = np.nonzero(ch)[0]
    want_kept = m0.match_kept_frames(sel)
    m0.gate_reset()
    want_gated = m0.match_changed_frames(useq)
    assert g.match_frames(frames).tobytes() == want.tobytes()
    assert [g.last_candidates(i).tobytes() for i in range(len(frames))] == cands
    gc, gs, gl = g.changed_mask(seq)
    assert np.array_equal(gc, ch) and gs.tobytes() == sim.tobytes() and np.array_equal(gl, last)
    assert g.match_kept_frames(sel).tobytes() == want_kept.tobytes()
    assert _same3(g.match_changed_frames(seq), want_gated)
    # a refused lens changes no member
    assert _code(capi, lambda: g.set_frame_lens(SRC[0], SRC[1], k1=-0.5))[0] == 1
    assert g.member(0).frame_lens == LENS and g.member(1).frame_lens == LENS
    g.clear_frame_lens()
    assert g.frame_lens is None
    assert g.match_frames(und).tobytes() == want.tobytes()
    g.close(); m0.close()


def test_lens_with_a_region_a_mask_shading_and_levels(capi, deck):
    pages, (frames, _) = deck
    mw, m0 = _matcher(capi, pages, region=True), _matcher(capi, pages, lens=False)
    M = capi.frame_region_from_quad(QUAD, *OUT)
    und = _und(mw, frames)
    assert np.array_equal(und[0], FL.undistort(frames[0], LENS[2:], M, *OUT)), "the tap under lens and region"
    assert np.array_equal(mw.rectify(frames[0]), R.rectify(frames[0], M, *OUT)), "the region's own tap"
    plain = _trace(m0, m0.match_frames(und))
    _paged(np.frombuffer(plain[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == plain, "lens + region"
    # a frame mask of the analysed size
    mask = np.full((OUT[1], OUT[0]), 255, np.uint8)
    mask[-150:, -240:] = 0
    mw.set_frame_mask(mask); m0.set_frame_mask(mask)
    want = _trace(m0, m0.match_frames(und))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert want != plain
    assert _trace(mw, mw.match_frames(frames)) == want, "a frame mask"
    mw.set_frame_mask(None); m0.set_frame_mask(None)
    # shading and levels behind the lens
    gw, gh = SR.grid(OUT[0], OUT[1], 32)
    j, i = np.mgrid[0:gh + 1, 0:gw + 1].astype(np.float64)
    gains = np.rint(256 * (0.8 + 0.4 * (((i * 32 - OUT[0] / 2) / (OUT[0] / 2)) ** 2 + ((j * 32 - OUT[1] / 2) / (OUT[1] / 2)) ** 2))).astype(np.uint16)
    lut = np.stack([np.clip(np.arange(256) * g + o, 0, 255).astype(np.uint8) for g, o in ((0.9, 10), (1.05, -5), (0.95, 3))])
    mw.set_frame_shading(OUT[0], OUT[1], 32, gains); mw.set_frame_levels(lut)
    both = LR.apply(SR.apply(und, 32, gains), lut)
    want = _trace(m0, m0.match_frames(both))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == want, "shading and levels follow the lens"
    mw.close(); m0.close()


def _mode_equal(capi, deck, n=8, prepare=None, **kw):
    pages, (frames, _) = deck
    frames = frames[:n]
    mw, m0 = _matcher(capi, pages, **kw), _matcher(capi, pages, lens=False, **kw)
    if prepare:
        prepare(mw); prepare(m0)
    want = _trace(m0, m0.match_frames(_und(mw, frames)))
    _paged(np.frombuffer(want[0], capi.VERDICT_DTYPE))
    assert _trace(mw, mw.match_frames(frames)) == want
    mw.close(); m0.close()


def test_mode_homography(capi, deck):
    _mode_equal(capi, deck, verify_model=1)


def test_mode_ratio_test(capi, deck):
    _mode_equal(capi, deck, ratio_test=0.97)


def test_mode_page_set(capi, deck):
    sel = sorted(set(int(t) for t in deck[1][1]))                 # the pages the frames show (every frame keeps its page in the set)
    assert 1 <= len(sel) <= 6
    _mode_equal(capi, deck, prepare=lambda m: m.use_page_set(m.create_page_set(sel)))


def test_mode_sift(capi, deck):
    _mode_equal(capi, deck, n=4, sift=(capi.sift_config(nfeatures=1000), 0.0))


# ---- errors, refusals, the off value -----------------------------------------------------------------------------------------------

def test_errors_and_refusals(capi, deck):
    pages, (frames, _) = deck
    frames = frames[:2]
    m = _matcher(capi, pages, lens=False)
    cx, cy, f = FL.defaults(*SRC)

    def set_(sw, sh, cx_=cx, cy_=cy, f_=f, k1=-0.08, k2=0.0):
        return _code(capi, lambda: m.set_frame_lens(sw, sh, cx_, cy_, f_, k1, k2))
    # set-time refusals, the rule named, nothing set
    for sw, sh in ((0, 540), (960, 0), (4097, 540), (960, 4097), (-1, -1)):
        c, msg = set_(sw, sh)
        assert c == 1 and "source size" in msg, msg
    for kw in (dict(cx_=float("nan")), dict(cy_=float("inf")), dict(f_=float("nan")), dict(k1=float("inf")), dict(k2=float("nan"))):
        c, msg = set_(*SRC, **kw)
        assert c == 1 and "finite" in msg, msg
    for bad in (0.0, -3.0):
        c, msg = set_(*SRC, f_=bad)
        assert c == 1 and "positive" in msg, msg
    for k1, k2 in ((-0.34, 0.0), (-1.5, 1.0), (0.2, -0.5)):
        c, msg = set_(*SRC, k1=k1, k2=k2)
        assert c == 1 and "increasing" in msg, msg
    assert m.frame_lens is None
    # the reach is the region's in force, in both orders: a quad that reaches r2 = 2.2 under k1 = -0.3
    wide = [(-240.0, -135.0), (1199.0, -135.0), (1199.0, 674.0), (-240.0, 674.0)]
    m.set_frame_lens(*SRC, k1=-0.3)
    c, msg = _code(capi, lambda: m.set_frame_region(SRC[0], SRC[1], wide, *OUT))
    assert c == 1 and "increasing" in msg and m.frame_region is None
    m.clear_frame_lens()
    m.set_frame_region(SRC[0], SRC[1], wide, *OUT)
    c, msg = set_(*SRC, k1=-0.3)
    assert c == 1 and "increasing" in msg and m.frame_lens is None
    # a lens and a region of different source sizes, in both orders
    c, msg = set_(1920, 1080, 959.5, 539.5, 2 * f)
    assert c == 5 and "1920x1080" in msg and "960x540" in msg and m.frame_lens is None
    m.clear_frame_region()
    m.set_frame_lens(1920, 1080, 959.5, 539.5, 2 * f, -0.08, 0.0)
    c, msg = _code(capi, lambda: m.set_frame_region(SRC[0], SRC[1], QUAD, *OUT))
    assert c == 5 and "1920x1080" in msg and "960x540" in msg and m.frame_region is None
    # a frame call at another source size names both sizes; nothing is silently left distorted
    for fn in (lambda: m.match_frames(frames), lambda: m.changed_mask(frames), lambda: m.match_changed_frames(frames),
               lambda: m.gate_reset_from_frame(frames[0]), lambda: m.undistort(frames[0])):
        c, msg = _code(capi, fn)
        assert c == 1 and "1920x1080" in msg and "960x540" in msg, msg
    # the working size, in both orders: a lens without a region analyses at its source size, which must fit
    m.set_frame_lens(*LENS)
    c, msg = _code(capi, lambda: m.set_working_size(640, 360))
    assert c == 5 and "640x360" in msg and "960x540" in msg and m.working_size == (0, 0)
    m.set_working_size(960, 540)
    want = m.match_frames(frames).tobytes()
    m.set_working_size(0, 0)
    assert m.match_frames(frames).tobytes() == want
    m.clear_frame_lens()
    m.set_working_size(640, 360)
    c, msg = set_(*SRC)
    assert c == 5 and "640x360" in msg and "960x540" in msg and m.frame_lens is None
    m.set_frame_region(SRC[0], SRC[1], QUAD, 640, 360)            # beside a region the region's output is what fits
    m.set_frame_lens(*LENS)
    assert m.undistort(frames[0]).shape == (360, 640, 3)
    m.clear_frame_lens(); m.clear_frame_region(); m.set_working_size(0, 0)
    # small_area refers to the analysed size
    m.set_frame_region(SRC[0], SRC[1], QUAD, 320, 180)
    m.set_frame_lens(*LENS)
    c, msg = _code(capi, lambda: m.match_frames(frames))
    assert c == 5 and "320x180" in msg, msg
    assert m.undistort(frames[0]).shape == (180, 320, 3)           # (the tap applies no such limit)
    m.clear_frame_lens(); m.clear_frame_region()
    # a frame mask and a shading field of another size than the analysed one
    m.set_frame_lens(*LENS)
    m.set_frame_mask(np.full((360, 640), 255, np.uint8))
    assert _code(capi, lambda: m.match_frames(frames))[0] == 1
    m.set_frame_mask(None)
    # the tap without a lens
    m.clear_frame_lens()
    assert _code(capi, lambda: m.undistort(frames[0]))[0] == 4
    m.close()


def test_the_use(capi, synth):
    """The keystone scene bent by k1 = -0.08 (tests/frame_lens_ref.py use_scene) at placement_ref.USE's session: the session's sums
    are the restatement's integers on the library's own features and traces, hence the same fit — the learner's lens and quad are
    frame_lens_ref.placement_lens's of those sums —; the largest corner error and the displacement error at the frame's corner are
    within the bounds test_frame_lens_abi.py test_the_use_on_the_cpu records; the setter takes the learnt lens beside the learnt quad,
    and every frame that keeps its page with nothing set keeps it under them.  (Whether the mean winning inliers rise over the quad
    alone is printed, not asserted: on the CPU they do not.)"""
    import evidence_ref as E
    import placement_ref as P
    from conftest import small_cfg
    from slideo_amd import matching
    pages, frames, truth, lens = FL.use_scene(synth)
    U = P.USE
    aw, ah = E.CANVAS_W, E.CANVAS_H
    cfg = small_cfg(capi, nfeatures=U["nfeatures"], min_rating=U["min_rating"])
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    before = m.match_frames(frames)
    # the sums of the session are the restatement's
    m.placement_begin(U["cell"], U["min_inliers"], U["reach"])
    m.match_frames(frames)
    sums, through, counted = m.placement_sums()
    m.placement_end()
    train = np.concatenate([d for _, d in [m.page_features(p) for p in range(m.page_count)]])
    tp, pxy = E.deck_of(m, m.page_count)
    sizes = {p: (pg.shape[1], pg.shape[0]) for p, pg in enumerate(pages)}
    m.match_frames(frames)                                      # (the traces of the same call, outside the session)
    recs = []
    for i, fr in enumerate(frames):
        kp, desc = m.orb(fr)
        recs.append(P.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, m.last_candidates(i), train))
    want = P.sums(recs, cell=U["cell"], aw=aw, ah=ah, min_inliers=U["min_inliers"], reach=U["reach"], model=0, train_page=tp, page_xy=pxy, page_sizes=sizes,
                  guard=False)
    assert (through, counted) == want[1:] and np.array_equal(sums, want[0])
    for order in (1, 2):
        kw = dict(cell=U["cell"], min_inliers=U["min_inliers"], reach=U["reach"], min_count=U["min_count"], trim_px=U["trim"], rounds=U["rounds"], order=order)
        learnt, quad = matching.learn_frame_lens_from_matches(m, [frames[:4], frames[4:]], **kw)
        assert pytest.raises(capi.SlideoError, m.placement_info).value.code == 4          # the learner ends its session
        assert learnt[:5] == (aw, ah) + lens[:3] and m.frame_lens is None and m.frame_region is None, "the defaults; nothing is installed"
        ref = FL.placement_lens(sums, U["cell"], aw, ah, U["min_count"], *lens[:3], order, U["trim"], U["rounds"], FL.USE_ITERS, guard=False)
        assert ref is not None and np.abs(np.array(quad) - ref["quad"]).max() <= 1e-3
        k = learnt[5:]
        assert abs(FL.displacement(lens[2], *k, ref["R2"]) - FL.displacement(lens[2], *ref["k"], ref["R2"])) <= 1e-3
        err, derr = P.corner_error(quad), FL.corner_displacement_error(lens, k, aw, ah)
        B = FL.USE_BOUNDS[order]
        ow, oh = FL.out_size_of(quad)
        m.set_frame_region(aw, ah, quad, ow, oh)
        quad_alone = m.match_frames(frames)                       # (the quad in ideal coordinates without its lens: for the record only)
        m.set_frame_lens(*learnt)
        try:
            after = m.match_frames(frames)
        finally:
            m.clear_frame_lens(); m.clear_frame_region()
        print("the use, order %d: %d of %d frames contribute; k (%.4f, %.4f); largest corner error %.2f px (bound %.0f); displacement error at the frame "
              "corner %.2f px (bound %.0f); region %dx%d; pages kept %d with nothing set, %d under lens and quad; mean winning inliers %.1f, %.1f (the "
              "ideal quad without the lens: %.1f)" % (order, counted, through, k[0], k[1], err, B["corner_px"], derr, B["corner_disp_px"], ow, oh,
                                                       int((before["page_idx"] >= 0).sum()), int((after["page_idx"] >= 0).sum()), before["inliers"].mean(),
                                                       after["inliers"].mean(), quad_alone["inliers"].mean()))
        assert err <= B["corner_px"] and derr <= B["corner_disp_px"]
        had = before["page_idx"] >= 0
        assert had.any() and np.array_equal(after["page_idx"][had], before["page_idx"][had])
    with pytest.raises(ValueError, match="is set"):
        m.set_frame_lens(aw, ah, k1=-0.05)
        try:
            matching.learn_frame_lens_from_matches(m, [frames[:2]], **kw)
        finally:
            m.clear_frame_lens()
    with pytest.raises(ValueError, match="no frame was matched"):
        matching.learn_frame_lens_from_matches(m, [], **kw)
    m.close()


def test_the_off_value_launches_what_no_lens_launches(capi, deck):
    """set(k = 0) reports is_set == 0 whatever else is given, and every byte is what it is with no lens set: without a region the
    frames are analysed as they lie (no rectify launch: a device call at another size than the "lens's" passes), with one the region's
    own instance runs (the rectify tap's image, column-block term included)."""
    pages, (frames, _) = deck
    frames = frames[:4]
    m, m0 = _matcher(capi, pages, lens=False), _matcher(capi, pages, lens=False)
    m.set_frame_lens(*LENS)
    m.set_frame_lens(0, -5, float("nan"), float("nan"), -1.0, 0.0, 0.0)
    assert m.frame_lens is None
    want = _trace(m0, m0.match_frames(frames))
    assert _trace(m, m.match_frames(frames)) == want
    small = np.ascontiguousarray(frames[:, :450, :800])
    assert m.match_frames(small).tobytes() == m0.match_frames(small).tobytes(), "no lens: no source-size rule"
    assert _code(capi, lambda: m.undistort(frames[0]))[0] == 4
    for x in (m, m0):
        x.set_frame_region(SRC[0], SRC[1], QUAD, *OUT)
    m.set_frame_lens(*LENS)
    m.set_frame_lens(*SRC, k1=0.0, k2=0.0)
    assert m.frame_lens is None and m.frame_region is not None
    rect = np.stack([m.rectify(f) for f in frames])
    assert np.array_equal(rect[0], R.rectify(frames[0], capi.frame_region_from_quad(QUAD, *OUT), *OUT))
    assert _trace(m, m.match_frames(frames)) == _trace(m0, m0.match_frames(frames))
    m.close(); m0.close()
