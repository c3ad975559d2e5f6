"""Match shading map (include/slideo_amd.h "Match shading map") on the GPU: shading_map_kernel's sums, bit for bit against
tests/shading_ref.py (whose sampler is tone_ref's, 1e-9 guards included) on the tone table's constructed cases at cells 16, 32 and 64
and on ORB's own features (cfg0_data); the same sums from every call form that runs the verify stage; beside a working size and the
other three sessions; no double counting when a unit is run again; the session's rules and limits; and the use: a field learnt from
frames under a falloff that brings every one of them back to its page."""
import ctypes as C

import numpy as np
import pytest

import evidence_ref as E
import shading_ref as R
import tone_ref as T
import verify_cases as VC
from conftest import small_cfg

pytestmark = pytest.mark.gpu

W, H = 640, 360
S0 = (32, 8, 8, 255)      # the session of the cfg0 tests: cell, min_inliers, min_hits, flat


def _features_matcher(capi, case, cfg):
    """-> (matcher, {page: (w, h, small)})."""
    m = capi.Matcher(cfg)
    pages = {}
    for i, p in enumerate(case.pages):
        w, h = T.page_size(case, i)
        small = m.small_image(T.page_pixels(case, i))
        pages[i] = (w, h, small)
        m.add_page_features(w, h, VC.keypoints(p.xy), p.desc, small)
    m.finalize()
    return m, pages


def _inputs(case):
    n = len(case.frames)
    return np.stack([case.frame_pixels(i) for i in range(n)]), [VC.keypoints(f.xy) for f in case.frames], [f.desc for f in case.frames]


def _session(m, settings, call):
    """(what `call` returns, sums [3, gh, gw], frames_through, frames_counted) of one session around call()."""
    m.shading_begin(*settings)
    try:
        out = call()
        return (out,) + m.shading_sums()
    finally:
        m.shading_end()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


@pytest.mark.parametrize("cell", R.CELLS)
@pytest.mark.parametrize("entry", T.constructed_cases(), ids=lambda e: e[0])
def test_sums_equal_restatement_on_constructed_features(capi, entry, cell):
    """tone_ref.constructed_cases says what each case is there for; the restatement's sampler asserts the tone table's guards."""
    name, fa, pset, min_inliers, min_hits, flats = entry
    case = VC.build(*fa)
    cfg = small_cfg(capi, **case.cfg)
    m, pages = _features_matcher(capi, case, cfg)
    train, tp, pxy = case.deck()
    rows = None
    if pset is not None:
        m.use_page_set(m.create_page_set(pset))
        rows = np.nonzero(np.isin(tp, pset))[0]
    frames, kps, descs = _inputs(case)
    plain = m.match_features(frames, kps, descs)
    for flat in sorted(set(flats) | {0, 8, 255}):
        v, got, through, counted = _session(m, (cell, min_inliers, min_hits, flat), lambda: m.match_features(frames, kps, descs))
        assert v.tobytes() == plain.tobytes()                   # verdict bytes are identical with and without a session
        recs = [T.frame_record(cfg, f.xy, f.desc, m.last_candidates(i), train, frames[i], rows) for i, f in enumerate(case.frames)]
        want = R.sums(recs, cell, min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=cfg.verify_model, thr=cfg.ransac_threshold,
                      train_page=tp, page_xy=pxy, pages=pages)
        print("%s cell %d flat %d: %d through, %d counted, %d samples in %d cells" % (name, cell, flat, through, counted, got[0].sum(), (got[0] > 0).sum()))
        assert (through, counted) == want[1:], name
        assert got.shape == want[0].shape == (3,) + R.grid(W, H, cell)[::-1]
        assert np.array_equal(got, want[0]), (name, cell, flat, np.argwhere(got != want[0])[:4])
        if name in ("T2-inliers", "T2-hits"):
            assert counted == 0 and not got.any()
        elif flat == 255:
            assert counted >= 1 and got[0].sum() > 0 and (got[0] > 0).sum() > 1
    m.close()


@pytest.fixture(scope="module")
def cfg0(capi, cfg0_data):
    """The matcher of cfg0_data, its deck as tone_ref takes it, and the sync host call's session S0 (computed once, shared, left
    unchanged)."""
    pages, frames, truth, _ = cfg0_data
    cfg = small_cfg(capi)
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    plain = m.match_frames(frames)
    sync = _session(m, S0, lambda: m.match_frames(frames))
    feats = [m.page_features(p) for p in range(m.page_count)]
    tp, pxy = E.deck_of(m, m.page_count)
    deck = dict(train=np.concatenate([d for _, d in feats]), tp=tp, pxy=pxy,
                pages={p: (pages[p].shape[1], pages[p].shape[0], m.page_small(p)) for p in range(m.page_count)})
    yield m, cfg, frames, plain, sync, deck
    m.close()


def _ref_of_call(m, cfg, deck, analysed, call, settings=S0, knn_tap=False):
    """shading_ref's sums of `call` (a match call, run outside a session for its traces) whose analysed images are `analysed`."""
    import verify_ref as VR
    call()
    recs = []
    for i, img in enumerate(analysed):
        kp, desc = m.orb(img)
        votes = None
        if knn_tap and len(desc):
            idx, dist = m.knn(desc, deck["train"], cfg.knn_k)
            votes = VR.vote(cfg, idx.astype(np.int64), dist.astype(np.int64))
        recs.append(T.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, m.last_candidates(i), deck["train"], img, votes=votes))
    return R.sums(recs, settings[0], min_inliers=settings[1], min_hits=settings[2], flat=settings[3], model=cfg.verify_model,
                  thr=cfg.ransac_threshold, train_page=deck["tp"], page_xy=deck["pxy"], pages=deck["pages"], guard=False)


def test_sync_sums_equal_restatement_on_orb_features(capi, cfg0):
    m, cfg, frames, plain, sync, deck = cfg0
    v, got, through, counted = sync
    assert v.tobytes() == plain.tobytes()
    want = _ref_of_call(m, cfg, deck, frames, lambda: m.match_frames(frames))
    print("cfg0: %d through, %d counted, %d samples" % (through, counted, got[0].sum()))
    assert (through, counted) == want[1:] and counted >= 6
    assert np.array_equal(got, want[0]) and got[0].sum() > 100000
    for cell, flat in ((16, 0), (64, 8)):
        s = (cell, S0[1], S0[2], flat)
        a = _session(m, s, lambda: m.match_frames(frames))
        want = _ref_of_call(m, cfg, deck, frames, lambda: m.match_frames(frames), s)
        assert np.array_equal(a[1], want[0]) and a[3] == want[2] and 0 < a[1][0].sum() < got[0].sum()


def test_every_path_gives_the_same_sums(capi, cfg0, cfg0_data):
    import torch
    import yuv420_ref as Y
    m, cfg, frames, plain, sync, deck = cfg0
    n = len(frames)
    fb = W * H * 3
    t = torch.from_numpy(frames).cuda()
    assert _same(_session(m, S0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H)), sync)
    def stream():                                               # four units in flight on one set of accumulators
        tickets = [m.submit_dev(t.data_ptr() + 2 * i * fb, 2, W, H) for i in range(4)]
        assert m.shading_info()["frames_through"] == 0          # (the frames are those of the collected units)
        assert pytest.raises(capi.SlideoError, m.shading_sums).value.code == 4
        return np.concatenate([m.collect(x) for x in tickets])
    got = _session(m, S0, stream)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    def kept():
        m.changed_mask(frames)
        return m.match_kept_frames(np.arange(n))
    got = _session(m, S0, kept)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    def gated():                                                # every frame twice: the second of each pair is unchanged and adds nothing
        m.gate_reset(None)
        ch, _, v = m.match_changed_frames(np.repeat(frames, 2, 0))
        assert list(ch) == [True, False] * n
        return v[::2]
    got = _session(m, S0, gated)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    L, nb = capi.yuv420_layout("nv12", W, H)
    yuv = Y.frames_to_yuv(frames[2:5], L, nb)
    bgr = np.stack([Y.to_bgr(f, W, H, L) for f in yuv])
    got = _session(m, S0, lambda: m.match_frames_yuv420(yuv, W, H, L))
    assert got[3] >= 2 and _same(got, _session(m, S0, lambda: m.match_frames(bgr)))
    g = capi.Group(cfg, devices=[0, 0])                         # a two-member group on device 0: the members' sums
    g.add_pages(list(cfg0_data[0])); g.finalize()
    got = _session(g, S0, lambda: g.match_frames(frames))
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    g.close()


def test_beside_a_working_size_a_region_and_the_other_sessions(capi, cfg0):
    import torch
    m, cfg, frames, plain, sync, deck = cfg0
    n = len(frames)
    t = torch.from_numpy(frames).cuda()
    settings = [("working size", lambda: m.set_working_size(480, 270), lambda: m.set_working_size(0, 0), lambda: [m.reduce(f, 480, 270) for f in frames]),
                ("frame region", lambda: m.set_frame_region(W, H, [(30.5, 20.25), (600.0, 12.5), (610.75, 338.0), (15.0, 330.5)], 402, 300),
                 m.clear_frame_region, lambda: [m.rectify(f) for f in frames])]
    for name, on, off, analysed in settings:
        m.shading_begin(*S0)
        on()
        assert pytest.raises(capi.SlideoError, m.shading_info).value.code == 4, name      # the analysed image is another: the state "none"
        try:
            imgs = analysed()
            host = _session(m, S0, lambda: m.match_frames(frames))
            dev = _session(m, S0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H))
            want = _ref_of_call(m, cfg, deck, imgs, lambda: m.match_frames(frames))
        finally:
            off()
        assert host[3] >= 3 and _same(host, dev), name
        assert np.array_equal(host[1], want[0]) and host[2:] == want[1:], name
    # the other three sessions open beside it change nothing on either side
    alone = {}
    for k, begin, read, end in (("evidence", lambda: m.evidence_begin(32, 0), m.evidence_counts, m.evidence_end),
                                ("tone", lambda: m.tone_begin(8, 8, 255), m.tone_counts, m.tone_end),
                                ("placement", lambda: m.placement_begin(32, 8, 6.0), m.placement_sums, m.placement_end)):
        begin(); m.match_frames(frames); alone[k] = read(); end()
    m.evidence_begin(32, 0); m.tone_begin(8, 8, 255); m.placement_begin(32, 8, 6.0); m.shading_begin(*S0)
    v = m.match_frames(frames)
    both = dict(evidence=m.evidence_counts(), tone=m.tone_counts(), placement=m.placement_sums())
    got = (v,) + m.shading_sums()
    m.evidence_end(); m.tone_end(); m.placement_end()
    assert m.shading_info()["frames_through"] == n                 # the others' ends leave it open
    m.shading_end()
    assert v.tobytes() == plain.tobytes() and _same(got, sync)
    for k in alone:
        for a, b in zip(alone[k], both[k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), k


def test_a_unit_that_is_run_again_counts_once(capi, monkeypatch, cfg0, cfg0_data):
    import torch
    _, cfg, frames, plain, sync, deck = cfg0
    t = torch.from_numpy(frames).cuda()
    monkeypatch.setenv("SLIDEO_RNG_STREAM_LEN", "512")
    for path in ("sync", "submit"):
        m = capi.Matcher(cfg)
        m.add_pages(list(cfg0_data[0])); m.finalize()
        assert m.rng_stream_len() == 512
        if path == "sync":
            got = _session(m, S0, lambda: m.match_frames(frames))
        else:
            got = _session(m, S0, lambda: m.collect(m.submit_dev(t.data_ptr(), len(frames), W, H)))
        assert m.rng_stream_len() > 512, path                                      # the unit was run again
        assert got[0].tobytes() == plain.tobytes() and _same(got, sync), path
        m.close()
    monkeypatch.delenv("SLIDEO_RNG_STREAM_LEN")


def test_rules_and_limits(capi, cfg0, monkeypatch):
    import torch
    m, cfg, frames, plain, sync, deck = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    none = lambda: code(m.shading_info) == 4 and code(m.shading_sums) == 4
    for bad in ((24, 0, 1, 255), (32, -1, 1, 255), (32, 0, 0, 255), (32, 0, 1, -1), (32, 0, 1, 256)):
        assert code(lambda: m.shading_begin(*bad)) == 1 and none()
    m.shading_end()                                                                   # (fine in the state "none")
    m.shading_begin(16, 5, 7, 9)
    assert code(lambda: m.shading_begin(*S0)) == 4                                    # a session is open, and stays as it is
    assert m.shading_info() == dict(cell=16, min_inliers=5, min_hits=7, flat=9, aw=0, ah=0, gw=0, gh=0, frames_through=0)
    s, through, counted = m.shading_sums()
    assert s.shape == (3, 0, 0) and (through, counted) == (0, 0)
    m.shading_end()
    assert none()
    # begin under a set field and under a set table
    g = R.ramp_field(W, H, 32)
    m.set_frame_shading(W, H, 32, g)
    with pytest.raises(capi.SlideoError) as e:
        m.shading_begin(*S0)
    assert e.value.code == 4 and "frame shading is set" in str(e.value) and none()
    m.set_frame_shading(gains=None)
    m.set_frame_levels(np.tile(np.arange(256)[::-1].astype(np.uint8), (3, 1)))
    with pytest.raises(capi.SlideoError) as e:
        m.shading_begin(*S0)
    assert e.value.code == 4 and "field first and the table second" in str(e.value) and none()
    m.set_frame_levels(None)
    # the first counted call fixes the size; a call at another size is refused, both sizes named; the session stays
    m.shading_begin(*S0)
    m.match_frames(frames[:3])
    a = m.shading_sums()
    assert a[0].any() and a[1] == 3 and m.shading_info()["gw"] == 20 and m.shading_info()["gh"] == 12
    with pytest.raises(capi.SlideoError) as e:
        m.match_frames(np.zeros((1, 450, 800, 3), np.uint8))
    assert e.value.code == 1 and "800x450" in str(e.value) and "640x360" in str(e.value)
    assert m.shading_info()["frames_through"] == 3
    cap = np.zeros(10, np.uint64)
    gw, gh, ft, fc = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    p = cap.ctypes.data_as(C.c_void_p)
    assert capi.lib().slideo_matcher_shading_sums(m._h, p, p, p, C.c_int64(10), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)) == 7
    assert (gw.value, gh.value) == (20, 12) and not cap.any()
    assert capi.lib().slideo_matcher_shading_sums(m._h, p, None, p, C.c_int64(240), C.byref(gw), C.byref(gh), C.byref(ft), C.byref(fc)) == 1
    m.set_frame_mask(np.full((H, W), 255, np.uint8))                                   # the frame mask leaves the session open
    assert m.shading_info()["frames_through"] == 3
    m.set_frame_mask(None)
    m.set_frame_shading(W, H, 32, g)                                                   # the shading's own setter ends it
    assert none()
    m.set_frame_shading(gains=None)
    # the 4096-cell refusal, at the first counted call: 1040x1040 at cell 16 is 65 x 65 cells
    m.shading_begin(16, 0, 1, 255)
    with pytest.raises(capi.SlideoError) as e:
        m.match_frames(np.zeros((1, 1040, 1040, 3), np.uint8))
    assert e.value.code == 5 and "cell 32" in str(e.value) and m.shading_info()["aw"] == 0
    m.shading_end()
    # units in flight: no begin, no end
    t = torch.from_numpy(frames).cuda()
    ticket = m.submit_dev(t.data_ptr(), 2, W, H)
    assert code(lambda: m.shading_begin(*S0)) == 4 and code(m.shading_end) == 4
    m.collect(ticket)
    # the frames limit, lowered to 10 (SLIDEO_SHADING_MAX_FRAMES, read at begin): frames through, in flight and the call's own count
    monkeypatch.setenv("SLIDEO_SHADING_MAX_FRAMES", "10")
    m.shading_begin(*S0)
    monkeypatch.delenv("SLIDEO_SHADING_MAX_FRAMES")
    assert code(lambda: m.match_frames(np.concatenate([frames, frames[:3]]))) == 1    # 11 frames at once
    assert m.shading_info()["frames_through"] == 0
    a = m.submit_dev(t.data_ptr(), 4, W, H)
    b = m.submit_dev(t.data_ptr(), 4, W, H)
    with pytest.raises(capi.SlideoError) as e:                                        # 8 in flight + 3
        m.submit_dev(t.data_ptr(), 3, W, H)
    assert e.value.code == 1 and "11 frames" in str(e.value)
    m.collect(a); m.collect(b)
    assert m.shading_info()["frames_through"] == 8
    assert code(lambda: m.match_frames(frames[:3])) == 1
    m.match_frames(frames[:2])
    m.shading_end()
    # SIFT mode, either order
    s = capi.Matcher(small_cfg(capi))
    s.shading_begin(*S0)
    assert code(lambda: s.use_sift(capi.sift_config(), 0.75)) == 5
    assert s.shading_info()["flat"] == 255
    s.shading_end()
    s.use_sift(capi.sift_config(), 0.75)
    assert code(lambda: s.shading_begin(*S0)) == 5
    s.close()
    # a group validates every member before it touches one
    grp = capi.Group(cfg, devices=[0, 0])
    grp.member(1).shading_begin(*S0)
    assert code(lambda: grp.shading_begin(*S0)) == 4
    assert code(grp.member(0).shading_info) == 4                                      # member 0 was not touched
    grp.member(1).shading_end()
    grp.shading_begin(64, 1, 2, 3)
    assert grp.shading_info()["cell"] == 64 and grp.member(1).shading_info()["flat"] == 3
    grp.shading_end()
    assert code(grp.shading_sums) == 4
    grp.close()


def test_the_use(capi, synth):
    """The canvas scene with the window under a radial falloff to 0.2 (shading_ref.USE) through
    matching.learn_frame_shading_from_matches.  Figures found on the MI355X are printed; the bounds are the issue's.
    Found: see docs/EXTENSIONS.md "Match shading map", The use."""
    from slideo_amd import matching
    U = R.USE
    pages, frames, truth = E.canvas_scene(synth)
    cfg = small_cfg(capi, nfeatures=E.SCENE["nfeatures"], min_rating=U["min_rating"])
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    kw = dict(cell=U["cell"], min_inliers=U["min_inliers"], min_hits=U["min_hits"], flat=U["flat"], min_count=U["min_count"], min_gain=U["min_gain"],
              max_gain=U["max_gain"], smooth=U["smooth"])
    dim = R.window_falloff(frames)
    halves = lambda f: [f[:len(f) // 2], f[len(f) // 2:]]
    clean = m.match_frames(frames)
    before = m.match_frames(dim)
    field = matching.learn_frame_shading_from_matches(m, halves(dim), **kw)
    assert pytest.raises(capi.SlideoError, m.shading_info).value.code == 4            # the learner ends its session; nothing is installed
    assert m.frame_shading() is None
    sums, through, counted = _session(m, (U["cell"], U["min_inliers"], U["min_hits"], U["flat"]), lambda: m.match_frames(dim))[1:]
    want = R.field(sums[0], sums[1], sums[2], U["cell"], U["min_count"], U["min_gain"], U["max_gain"], U["smooth"])
    assert field[:3] == (frames.shape[2], frames.shape[1], U["cell"]) and np.array_equal(field[3], want[0])
    m.set_frame_shading(*field)
    after = m.match_frames(dim)
    TU = T.USE
    lut = matching.learn_frame_levels_from_matches(m, halves(dim), min_inliers=TU["min_inliers"], min_hits=TU["min_hits"], flat=TU["flat"],
                                                   min_count=TU["min_count"])
    m.set_frame_levels(lut)
    both = m.match_frames(dim)
    m.set_frame_levels(None)
    m.set_frame_shading(gains=None)
    tone_only = matching.learn_frame_levels_from_matches(m, halves(dim), min_inliers=TU["min_inliers"], min_hits=TU["min_hits"], flat=TU["flat"],
                                                         min_count=TU["min_count"])
    m.set_frame_levels(tone_only)
    tone = m.match_frames(dim)
    m.set_frame_levels(None)
    cfield = matching.learn_frame_shading_from_matches(m, halves(frames), **kw)
    m.set_frame_shading(*cfield)
    cafter = m.match_frames(frames)
    m.close()
    right = lambda v: int((v["page_idx"] == truth).sum())
    sim = lambda v: (float(v["similarity"][v["page_idx"] == truth].min()), float(np.median(v["similarity"][v["page_idx"] == truth])))
    # the field's node error against 1 / falloff, over the nodes inside the window (recorded, not gated)
    cell, gains = U["cell"], field[3]
    j, i = np.mgrid[0:gains.shape[0], 0:gains.shape[1]]
    x, y = np.minimum(i * cell, frames.shape[2] - 1) - E.WIN_X, np.minimum(j * cell, frames.shape[1] - 1) - E.WIN_Y
    inside = (x >= 0) & (x < E.WIN_W) & (y >= 0) & (y < E.WIN_H)
    rho2 = (((x - (E.WIN_W - 1) / 2) / (E.WIN_W / 2)) ** 2 + ((y - (E.WIN_H - 1) / 2) / (E.WIN_H / 2)) ** 2) / 2
    err = ((gains / 256.0) * (1 - U["a"] * rho2) - 1)[inside]
    print("the use: clean %d of 16 (similarity min %.3f median %.3f); falloff %d (%.3f / %.3f); field %d (%.3f / %.3f); field + table %d (%.3f / %.3f); "
          "table alone %d (%.3f / %.3f); %d frames contributed, %d cells used; node error against 1 / falloff inside the window: median %+.3f, "
          "worst %+.3f; clean field gains %.2f..%.2f, %d of 16"
          % (right(clean), *sim(clean), right(before), *sim(before), right(after), *sim(after), right(both), *sim(both), right(tone), *sim(tone),
             counted, want[1], float(np.median(err)), float(err[np.argmax(np.abs(err))]), cfield[3].min() / 256, cfield[3].max() / 256, right(cafter)))
    assert right(before) <= 8
    assert counted >= 8
    assert right(after) == 16 and after["similarity"].min() >= 0.70
    assert right(both) == 16
    assert cafter["page_idx"].tolist() == clean["page_idx"].tolist()
