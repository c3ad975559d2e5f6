"""Match tone table (include/slideo_amd.h "Match tone table") on the GPU: tone_kernel's counts against tests/tone_ref.py on constructed
features (tests/verify_cases.py through Matcher.match_features) and on ORB's own (cfg0_data), the same counts from every call form
that runs the verify stage and under the settings that change the analysed image, no double counting when a unit is run again, the
session's rules, and the use: a table learnt from darkened frames that brings every one of them back to its page."""
import numpy as np
import pytest

import evidence_ref as E
import levels_ref as LR
import tone_ref as T
import verify_cases as VC
from conftest import small_cfg

pytestmark = pytest.mark.gpu

W, H = 640, 360
S0 = (8, 8, 255)          # the session of the cfg0 tests: min_inliers, min_hits, flat


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
    """(what `call` returns, cnt, sum, frames_through, frames_counted) of one session around call()."""
    m.tone_begin(*settings)
    try:
        out = call()
        return (out,) + m.tone_counts()
    finally:
        m.tone_end()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and tuple(a[3:]) == tuple(b[3:])


@pytest.mark.parametrize("entry", T.constructed_cases(), ids=lambda e: e[0])
def test_counts_equal_restatement_on_constructed_features(capi, entry):
    """tone_ref.constructed_cases says what each case is there for; tone_ref.counts asserts that no tested residual lies within 1e-9
    (relative) of the threshold and no X + 0.5, Y + 0.5 or box comparison within 1e-9 of an integer."""
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
    samples = {}
    for flat in flats:
        v, cnt, sm, through, counted = _session(m, (min_inliers, min_hits, flat), lambda: m.match_features(frames, kps, descs))
        assert v.tobytes() == plain.tobytes()                   # verdict bytes are identical with and without a session
        recs = [T.frame_record(cfg, f.xy, f.desc, m.last_candidates(i), train, frames[i], rows) for i, f in enumerate(case.frames)]
        stats = []
        want = T.counts(recs, min_inliers=min_inliers, min_hits=min_hits, flat=flat, model=cfg.verify_model, thr=cfg.ransac_threshold,
                        train_page=tp, page_xy=pxy, pages=pages, stats=stats)
        print("%s flat %d: %d frames through, %d counted, %d samples" % (name, flat, through, counted, cnt[0].sum()))
        assert (through, counted) == want[2:], name
        assert np.array_equal(cnt, want[0]) and np.array_equal(sm, want[1]), (name, flat)
        samples[flat] = int(cnt[0].sum())
    who = [None if s is None else s[3] for s in stats]
    if name in ("T2-inliers", "T2-hits"):
        assert counted == 0 and not cnt.any() and T.contributor(recs[0]["cands"], 0) >= 0
    else:
        assert counted >= 1 and samples[255] > 0
    if name == "D2-other":                                       # the contributor is the page with the most inliers, not the verdict's
        assert v["page_idx"][0] >= 0 and who[0] is not None and who[0] != v["page_idx"][0]
        assert samples[0] < samples[2] < samples[8] < samples[255]
    if name == "BLACK":
        assert v["page_idx"][0] == -1 and counted == 1 and int(cnt[:, 1:].sum()) == 0      # every sample of a black frame is 0
    if name == "OUT":
        n, (bx0, by0, bx1, by1), hits, page = stats[0]
        w, h, small = pages[page]
        x = ((np.arange(small.shape[1]) + 0.5) * w) / small.shape[1] - 0.5; y = ((np.arange(small.shape[0]) + 0.5) * h) / small.shape[0] - 0.5
        assert 0 < n < 0.95 * int(((x >= bx0) & (x <= bx1)).sum()) * int(((y >= by0) & (y <= by1)).sum())
    if name == "V5-set":
        assert set(v["page_idx"]) <= set(pset) and who[0] in pset
    if name == "V1-empty":
        assert any(len(f.xy) == 0 for f in case.frames) and counted == 4
    if name == "SIZES":
        assert who == [0, 1] and pages[0][2].shape != pages[1][2].shape and counted == 2
    for s in stats:                                              # every hit box clips its page
        if s is not None:
            assert 0 < s[1][0] and 0 < s[1][1] and s[1][2] < pages[s[3]][0] - 1 and s[1][3] < pages[s[3]][1] - 1
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
    """tone_ref's counts of `call` (a match call, run outside a session for its traces) whose analysed images are `analysed`.
    knn_tap: the neighbour lists of the votes from the library's exact search tap (ORB-3000 frames: numpy's take seconds each)."""
    import verify_ref as R
    call()
    recs = []
    for i, img in enumerate(analysed):
        kp, desc = m.orb(img)
        votes = None
        if knn_tap and len(desc):
            idx, dist = m.knn(desc, deck["train"], cfg.knn_k)
            votes = R.vote(cfg, idx.astype(np.int64), dist.astype(np.int64))
        recs.append(T.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, m.last_candidates(i), deck["train"], img, votes=votes))
    return T.counts(recs, min_inliers=settings[0], min_hits=settings[1], flat=settings[2], model=cfg.verify_model, thr=cfg.ransac_threshold,
                    train_page=deck["tp"], page_xy=deck["pxy"], pages=deck["pages"], guard=False)


def test_sync_counts_equal_restatement_on_orb_features(capi, cfg0):
    m, cfg, frames, plain, sync, deck = cfg0
    v, cnt, sm, through, counted = sync
    assert v.tobytes() == plain.tobytes()
    want = _ref_of_call(m, cfg, deck, frames, lambda: m.match_frames(frames))
    print("cfg0: %d through, %d counted, %d samples" % (through, counted, cnt[0].sum()))
    assert (through, counted) == want[2:] and counted >= 6
    assert np.array_equal(cnt, want[0]) and np.array_equal(sm, want[1]) and cnt[0].sum() > 100000
    for flat in (0, 8):
        got = _session(m, (S0[0], S0[1], flat), lambda: m.match_frames(frames))
        want = _ref_of_call(m, cfg, deck, frames, lambda: m.match_frames(frames), (S0[0], S0[1], flat))
        assert np.array_equal(got[1], want[0]) and np.array_equal(got[2], want[1]) and got[4] == want[3] and 0 < got[1][0].sum() < cnt[0].sum()


def test_every_path_gives_the_same_counts(capi, cfg0, cfg0_data):
    import torch
    import yuv420_ref as Y
    m, cfg, frames, plain, sync, deck = cfg0
    n = len(frames)
    fb = W * H * 3
    t = torch.from_numpy(frames).cuda()
    # a device call
    assert _same(_session(m, S0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H)), sync)
    # submit / collect with four units in flight on one set of accumulators
    def stream():
        tickets = [m.submit_dev(t.data_ptr() + 2 * i * fb, 2, W, H) for i in range(4)]
        assert m.tone_info()["frames_through"] == 0             # (the frames are those of the collected units)
        with pytest.raises(capi.SlideoError) as e:
            m.tone_counts()
        assert e.value.code == 4
        return np.concatenate([m.collect(x) for x in tickets])
    got = _session(m, S0, stream)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    # kept frames of a mask call
    def kept():
        m.changed_mask(frames)
        return m.match_kept_frames(np.arange(n))
    got = _session(m, S0, kept)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    # a gated call: every frame twice, the second of each pair is unchanged and adds nothing
    def gated():
        m.gate_reset(None)
        ch, _, v = m.match_changed_frames(np.repeat(frames, 2, 0))
        assert list(ch) == [True, False] * n
        return v[::2]
    got = _session(m, S0, gated)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    # one NV12 call: the counts of the BGR images the library makes of the frames
    L, nb = capi.yuv420_layout("nv12", W, H)
    yuv = Y.frames_to_yuv(frames[2:5], L, nb)                  # (three frames: the restated conversion takes its time)
    bgr = np.stack([Y.to_bgr(f, W, H, L) for f in yuv])
    got = _session(m, S0, lambda: m.match_frames_yuv420(yuv, W, H, L))
    assert got[4] >= 2 and _same(got, _session(m, S0, lambda: m.match_frames(bgr)))
    # a two-member group on device 0: the members' sums
    g = capi.Group(cfg, devices=[0, 0])
    g.add_pages(list(cfg0_data[0])); g.finalize()
    got = _session(g, S0, lambda: g.match_frames(frames))
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    g.close()


def test_settings_that_change_the_analysed_image(capi, cfg0):
    """A working size, a frame region and a levels table: the samples are taken from the image the pipeline analyses (the taps'
    reduce, rectify and the table applied), from the host and the device call alike.  Each setter ends an open session."""
    import torch
    m, cfg, frames, plain, sync, deck = cfg0
    n = len(frames)
    t = torch.from_numpy(frames).cuda()
    lut = LR.stretch_lut([20, 10, 30], [235, 250, 220])
    settings = [("working size", lambda: m.set_working_size(480, 270), lambda: m.set_working_size(0, 0), lambda: [m.reduce(f, 480, 270) for f in frames]),
                ("frame region", lambda: m.set_frame_region(W, H, [(30.5, 20.25), (600.0, 12.5), (610.75, 338.0), (15.0, 330.5)], 402, 300),
                 m.clear_frame_region, lambda: [m.rectify(f) for f in frames]),
                ("levels", lambda: m.set_frame_levels(lut), lambda: m.set_frame_levels(None), lambda: list(LR.apply(frames, lut)))]
    for name, on, off, analysed in settings:
        m.tone_begin(*S0)
        on()
        assert pytest.raises(capi.SlideoError, m.tone_info).value.code == 4, name      # the analysed image is another: the state "none"
        try:
            imgs = analysed()
            host = _session(m, S0, lambda: m.match_frames(frames))
            dev = _session(m, S0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H))
            want = _ref_of_call(m, cfg, deck, imgs, lambda: m.match_frames(frames))
        finally:
            off()
        print("%s: %d counted, %d samples" % (name, host[4], host[1][0].sum()))
        assert host[4] >= 3 and _same(host, dev), name
        assert np.array_equal(host[1], want[0]) and np.array_equal(host[2], want[1]) and host[3:] == want[2:], name
        assert not _same(host, sync), name


def test_a_unit_that_is_run_again_counts_once(capi, monkeypatch, cfg0, cfg0_data):
    """A matcher created with 512 pre-drawn RNG outputs.  Through the features tap, H1's five votes on one line sample far past them
    and the tap's loop runs its rows again; through match_frames and submit / collect, cfg0's candidates without a model do the
    same and unit_collect runs the unit again from its frames.  The stream's length shows that the re-run happened; the counts
    equal a default matcher's."""
    import torch
    case = VC.build(VC.h1, (1,))
    cfg = small_cfg(capi, **case.cfg)
    frames, kps, descs = _inputs(case)
    m, _ = _features_matcher(capi, case, cfg)
    want = _session(m, (0, 1, 255), lambda: m.match_features(frames, kps, descs))
    m.close()
    monkeypatch.setenv("SLIDEO_RNG_STREAM_LEN", "512")
    m, _ = _features_matcher(capi, case, cfg)
    assert m.rng_stream_len() == 512
    got = _session(m, (0, 1, 255), lambda: m.match_features(frames, kps, descs))
    assert m.rng_stream_len() > 512                                                # the unit was run again
    m.close()
    assert want[4] == 1 and want[1].any()
    assert got[0].tobytes() == want[0].tobytes() and _same(got, want)
    _, cfg, frames, plain, sync, deck = cfg0
    t = torch.from_numpy(frames).cuda()
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


def test_with_an_evidence_session_open_too(capi, cfg0):
    """Both sessions on one matcher give what each gives alone, and the verdict bytes are those of no session."""
    m, cfg, frames, plain, sync, deck = cfg0
    m.evidence_begin(32, 0)
    alone = (m.match_frames(frames),) + m.evidence_counts()
    m.evidence_end()
    m.evidence_begin(32, 0)
    m.tone_begin(*S0)
    v = m.match_frames(frames)
    ev, tone = m.evidence_counts(), m.tone_counts()
    m.evidence_end()
    assert m.tone_info()["frames_through"] == len(frames)            # evidence_end leaves the tone session open
    m.evidence_begin(32, 0)
    m.tone_end()
    assert m.evidence_info()["frames_through"] == 0                  # and tone_end an evidence session
    m.evidence_end()
    assert v.tobytes() == plain.tobytes() == alone[0].tobytes()
    assert np.array_equal(ev[0], alone[1]) and np.array_equal(ev[1], alone[2]) and ev[2:] == alone[3:]
    assert _same((v,) + tone, sync)


def test_rules(capi, cfg0, monkeypatch):
    import torch
    m, cfg, frames, plain, sync, deck = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    none = lambda: code(m.tone_info) == 4 and code(m.tone_counts) == 4
    for bad in ((-1, 1, 255), (0, 0, 255), (0, -5, 255), (0, 1, -1), (0, 1, 256)):
        assert code(lambda: m.tone_begin(*bad)) == 1 and none()
    m.tone_end()                                                                      # (fine in the state "none")
    m.tone_begin(5, 7, 9)
    assert code(lambda: m.tone_begin(*S0)) == 4                                       # a session is open, and stays as it is
    assert m.tone_info() == dict(min_inliers=5, min_hits=7, flat=9, frames_through=0)
    cnt, sm, through, counted = m.tone_counts()
    assert not cnt.any() and not sm.any() and (through, counted) == (0, 0)           # nothing counted after begin
    m.tone_end()
    assert none()
    m.tone_begin(*S0)
    m.match_frames(frames[:3])
    a = m.tone_counts()
    assert a[0].any() and a[2] == 3
    m.match_frames(np.zeros((1, 450, 800, 3), np.uint8))                              # another analysed size counts on
    assert m.tone_info()["frames_through"] == 4
    # the frame mask leaves the session open; a new session starts from zero
    m.set_frame_mask(np.full((H, W), 255, np.uint8))
    assert m.tone_info()["frames_through"] == 4
    m.set_frame_mask(None)
    m.tone_end()
    m.tone_begin(*S0)
    m.match_frames(frames[:3])
    b = m.tone_counts()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and b[2] == 3 and a[3] == b[3]
    m.set_working_size(0, 0)                                                          # a setter that changes the analysed image ends it
    assert none()
    # units in flight: no begin, no end
    t = torch.from_numpy(frames).cuda()
    ticket = m.submit_dev(t.data_ptr(), 2, W, H)
    assert code(lambda: m.tone_begin(*S0)) == 4 and code(m.tone_end) == 4
    m.collect(ticket)
    # the frames limit, lowered to 10 (SLIDEO_TONE_MAX_FRAMES, read at begin): frames through, in flight and the call's own count
    monkeypatch.setenv("SLIDEO_TONE_MAX_FRAMES", "10")
    m.tone_begin(*S0)
    monkeypatch.delenv("SLIDEO_TONE_MAX_FRAMES")
    assert code(lambda: m.match_frames(np.concatenate([frames, frames[:3]]))) == 1    # 11 frames at once
    assert m.tone_info()["frames_through"] == 0 and not m.tone_counts()[0].any()      # (refused before anything ran)
    a = m.submit_dev(t.data_ptr(), 4, W, H)
    b = m.submit_dev(t.data_ptr(), 4, W, H)
    with pytest.raises(capi.SlideoError) as e:                                        # 8 in flight + 3
        m.submit_dev(t.data_ptr(), 3, W, H)
    assert e.value.code == 1 and "11 frames" in str(e.value)
    m.collect(a); m.collect(b)
    assert m.tone_info()["frames_through"] == 8
    assert code(lambda: m.match_frames(frames[:3])) == 1
    m.match_frames(frames[:2])
    m.tone_end()
    # SIFT mode, either order
    s = capi.Matcher(small_cfg(capi))
    s.tone_begin(*S0)
    assert code(lambda: s.use_sift(capi.sift_config(), 0.75)) == 5
    assert s.tone_info()["flat"] == 255
    s.tone_end()
    s.use_sift(capi.sift_config(), 0.75)
    assert code(lambda: s.tone_begin(*S0)) == 5
    s.close()
    # a group validates every member before it touches one
    g = capi.Group(cfg, devices=[0, 0])
    g.member(1).tone_begin(*S0)
    assert code(lambda: g.tone_begin(*S0)) == 4
    assert code(g.member(0).tone_info) == 4                                           # member 0 was not touched
    assert code(g.tone_info) == 4
    g.member(1).tone_end()
    g.tone_begin(1, 2, 3)
    assert g.tone_info() == dict(min_inliers=1, min_hits=2, flat=3, frames_through=0) and g.member(1).tone_info()["flat"] == 3
    g.tone_end()
    assert code(g.tone_counts) == 4
    g.close()


@pytest.fixture(scope="module")
def use_scene(capi, synth):
    pages, frames, truth = E.canvas_scene(synth)
    cfg = small_cfg(capi, nfeatures=E.SCENE["nfeatures"], min_rating=T.USE["min_rating"])
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    yield m, cfg, pages, frames, truth
    m.close()


def test_the_use(capi, use_scene):
    """The darkened canvas scene (tests/test_tone_abi.py states it) through matching.learn_frame_levels_from_matches: the learnt table
    equals tone_ref's from the library's own traces, and with it installed every one of the 16 darkened frames gets its true page.
    While a table is set, the learner returns the composition with it."""
    from slideo_amd import matching
    m, cfg, pages, frames, truth = use_scene
    U = T.USE
    kw = dict(min_inliers=U["min_inliers"], min_hits=U["min_hits"], flat=U["flat"], min_count=U["min_count"])
    dark = T.darken(frames)
    batches = [dark[:len(dark) // 2], dark[len(dark) // 2:]]
    before = m.match_frames(dark)
    lut = matching.learn_frame_levels_from_matches(m, batches, **kw)
    assert pytest.raises(capi.SlideoError, m.tone_info).value.code == 4               # the learner ends its session
    feats = [m.page_features(p) for p in range(m.page_count)]
    tp, pxy = E.deck_of(m, m.page_count)
    deck = dict(train=np.concatenate([d for _, d in feats]), tp=tp, pxy=pxy,
                pages={p: (pages[p].shape[1], pages[p].shape[0], m.page_small(p)) for p in range(m.page_count)})
    settings = (U["min_inliers"], U["min_hits"], U["flat"])
    want = _ref_of_call(m, cfg, deck, dark, lambda: m.match_frames(dark), settings, knn_tap=True)
    assert want[3] >= 10
    assert np.array_equal(lut, T.lut(want[0], want[1], U["min_count"]))
    m.set_frame_levels(lut)
    try:
        after = m.match_frames(dark)
        # under the table, the learner sees levelled frames (test_settings_that_change_the_analysed_image holds those counts to
        # the restatement) and returns the composition with the table
        again = matching.learn_frame_levels_from_matches(m, batches, **kw)
        lev = _session(m, settings, lambda: m.match_frames(dark))
    finally:
        m.set_frame_levels(None)
    print("the use: %d of 16 right when darkened, %d with the learnt table (lowest similarity %.3f); %d frames contributed, %d samples"
          % ((before["page_idx"] == truth).sum(), (after["page_idx"] == truth).sum(), after["similarity"].min(), want[3], want[0][0].sum()))
    assert (after["page_idx"] == truth).all()
    second = T.lut(lev[1], lev[2], U["min_count"])
    assert np.array_equal(again, np.stack([second[c][lut[c]] for c in range(3)]))
    with pytest.raises(ValueError, match="contributed"):
        matching.learn_frame_levels_from_matches(m, [dark[:2]], **dict(kw, min_hits=10 ** 6))
    assert pytest.raises(capi.SlideoError, m.tone_info).value.code == 4               # a failed learner leaves no session open
