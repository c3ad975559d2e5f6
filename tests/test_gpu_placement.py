"""Match placement map (include/slideo_amd.h "Match placement map") on the GPU: placement_kernel's sums against tests/placement_ref.py on
constructed features (tests/verify_cases.py through Matcher.match_features) and on ORB's own (cfg0_data), the same sums from every
call form that runs the verify stage and beside open evidence and tone sessions, no double counting when a unit is run again, the
session's rules, and the use: a keystoned region learnt from the matches that is the scene's quad within the recorded bound."""
import numpy as np
import pytest

import evidence_ref as E
import placement_ref as P
import tone_ref as T
import verify_cases as VC
from conftest import small_cfg

pytestmark = pytest.mark.gpu

W, H = 640, 360
S0 = (32, 8, 6.0)         # the session of the cfg0 tests: cell, min_inliers, reach


def _features_matcher(capi, case, cfg):
    m = capi.Matcher(cfg)
    for i, p in enumerate(case.pages):
        w, h = T.page_size(case, i)
        m.add_page_features(w, h, VC.keypoints(p.xy), p.desc, m.small_image(T.page_pixels(case, i)))
    m.finalize()
    return m


def _inputs(case):
    n = len(case.frames)
    return np.stack([case.frame_pixels(i) for i in range(n)]), [VC.keypoints(f.xy) for f in case.frames], [f.desc for f in case.frames]


def _session(m, settings, call):
    """(what `call` returns, sums, frames_through, frames_counted) of one session around call()."""
    m.placement_begin(*settings)
    try:
        out = call()
        return (out,) + m.placement_sums()
    finally:
        m.placement_end()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


@pytest.mark.parametrize("entry", P.constructed_cases(), ids=lambda e: e[0])
def test_sums_equal_restatement_on_constructed_features(capi, entry):
    """placement_ref.constructed_cases says what each case is there for; placement_ref.sums asserts that no tested d2 lies within 1e-9
    (relative) of reach^2 or of a rival d2 of its keypoint.  Cells 16, 32 and 64 at a reach above ransac_threshold, cell 32 at one
    below."""
    name, fa, pset, min_inliers = entry
    case = VC.build(*fa)
    cfg = small_cfg(capi, **case.cfg)
    m = _features_matcher(capi, case, cfg)
    train, tp, pxy = case.deck()
    sizes = {i: T.page_size(case, i) for i in range(len(case.pages))}
    rows = None
    if pset is not None:
        m.use_page_set(m.create_page_set(pset))
        rows = np.nonzero(np.isin(tp, pset))[0]
    frames, kps, descs = _inputs(case)
    plain = m.match_features(frames, kps, descs)
    for cell, reach in ((16, P.REACHES[0]), (32, P.REACHES[0]), (64, P.REACHES[0]), (32, P.REACHES[1])):
        v, sums, through, counted = _session(m, (cell, min_inliers, reach), lambda: m.match_features(frames, kps, descs))
        assert v.tobytes() == plain.tobytes()
        recs = [P.frame_record(cfg, f.xy, f.desc, m.last_candidates(i), train, rows) for i, f in enumerate(case.frames)]
        stats = {}
        want = P.sums(recs, cell=cell, aw=W, ah=H, min_inliers=min_inliers, reach=reach, model=cfg.verify_model, train_page=tp, page_xy=pxy,
                      page_sizes=sizes, stats=stats)
        print("%s cell %d reach %g: %d through, %d counted, %d keypoints, %s" % (name, cell, reach, through, counted, sums[0].sum(), stats))
        assert (through, counted) == want[1:], name
        assert np.array_equal(sums, want[0]), (name, cell, reach)
        P.check_statements(name, reach, stats, sums, counted)
    m.close()


@pytest.fixture(scope="module")
def cfg0(capi, cfg0_data):
    """The matcher of cfg0_data and the sync host call's session (computed once, shared, left unchanged)."""
    pages, frames, truth, _ = cfg0_data
    cfg = small_cfg(capi)
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    plain = m.match_frames(frames)
    sync = _session(m, S0, lambda: m.match_frames(frames))
    yield m, cfg, frames, plain, sync
    m.close()


@pytest.mark.parametrize("cell", [16, 32, 64])
def test_sync_sums_equal_restatement_on_orb_features(capi, cfg0, cfg0_data, cell):
    m, cfg, frames, plain, sync = cfg0
    got = sync if cell == S0[0] else _session(m, (cell,) + S0[1:], lambda: m.match_frames(frames))
    v, sums, through, counted = got
    assert v.tobytes() == plain.tobytes()                       # verdict bytes are identical with and without a session
    feats = [m.page_features(p) for p in range(m.page_count)]
    train = np.concatenate([d for _, d in feats])
    tp, pxy = E.deck_of(m, m.page_count)
    sizes = {p: (pg.shape[1], pg.shape[0]) for p, pg in enumerate(cfg0_data[0])}
    m.match_frames(frames)                                      # (the traces of the same call, outside the session)
    recs = []
    for i, f in enumerate(frames):
        kp, desc = m.orb(f)
        recs.append(P.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, m.last_candidates(i), train))
    want = P.sums(recs, cell=cell, aw=W, ah=H, min_inliers=S0[1], reach=S0[2], model=0, train_page=tp, page_xy=pxy, page_sizes=sizes)
    print("cfg0 cell %d: %d through, %d counted, %d keypoints" % (cell, through, counted, sums[0].sum()))
    assert (through, counted) == want[1:] and counted >= 6
    assert np.array_equal(sums, want[0]) and sums[0].sum() > 100


def test_every_path_gives_the_same_sums(capi, cfg0, cfg0_data):
    import torch
    import yuv420_ref as Y
    m, cfg, frames, plain, sync = cfg0
    n = len(frames)
    fb = W * H * 3
    t = torch.from_numpy(frames).cuda()
    # a device call
    assert _same(_session(m, S0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H)), sync)
    # submit / collect with four units in flight on one accumulator
    def stream():
        tickets = [m.submit_dev(t.data_ptr() + 2 * i * fb, 2, W, H) for i in range(4)]
        assert m.placement_info()["frames_through"] == 0        # (the frame counts are those of the collected units)
        with pytest.raises(capi.SlideoError) as e:
            m.placement_sums()
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
    # ... with a direct similarity: frames that show a page full-screen are resolved directly and add nothing
    ys, xs = np.arange(H) * 450 // H, np.arange(W) * 800 // W
    pages = cfg0_data[0]
    full = np.stack([p[ys][:, xs] for p in pages[:2]])
    seq = np.concatenate([full, frames])
    m.set_direct_similarity(0.85)
    try:
        def direct():
            m.gate_reset(None)
            ch, _, v = m.match_changed_frames(seq)
            return ch, v
        (ch, v), sums, through, counted = _session(m, S0, direct)
    finally:
        m.set_direct_similarity(0.0)
    is_direct = ch & (v["page_idx"] >= 0) & (v["inliers"] == 0) & (v["n_keypoints"] == 0)
    assert is_direct.any() and through == int((ch & ~is_direct).sum()) and 0 < through < len(seq)
    rest = seq[ch & ~is_direct]
    assert _same(((), sums, through, counted), _session(m, S0, lambda: m.match_frames(rest)))
    # one NV12 call: the sums of the BGR images the library makes of the frames
    L, nb = capi.yuv420_layout("nv12", W, H)
    yuv = Y.frames_to_yuv(frames, L, nb)
    bgr = np.stack([Y.to_bgr(f, W, H, L) for f in yuv])
    assert _same(_session(m, S0, lambda: m.match_frames_yuv420(yuv, W, H, L)), _session(m, S0, lambda: m.match_frames(bgr)))
    # a two-member group on device 0: the members' sums
    g = capi.Group(cfg, devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    got = _session(g, S0, lambda: g.match_frames(frames))
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    assert g.placement_sums is not None
    g.close()


def test_three_sessions_side_by_side(capi, cfg0):
    """Evidence, tone and placement sessions open at once: each one's results are what they are alone."""
    m, cfg, frames, plain, sync = cfg0
    m.evidence_begin(32, 0)
    ev = (m.match_frames(frames),) + m.evidence_counts()
    m.evidence_end()
    m.tone_begin(8, 8, 255)
    tn = (m.match_frames(frames),) + m.tone_counts()
    m.tone_end()
    m.evidence_begin(32, 0); m.tone_begin(8, 8, 255); m.placement_begin(*S0)
    try:
        v = m.match_frames(frames)
        ev3, tn3, pl3 = m.evidence_counts(), m.tone_counts(), m.placement_sums()
    finally:
        m.placement_end(); m.tone_end(); m.evidence_end()
    assert v.tobytes() == plain.tobytes()
    assert _same((v,) + pl3, sync)
    assert all(np.array_equal(a, b) for a, b in zip(ev[1:3], ev3[:2])) and tuple(ev[3:]) == tuple(ev3[2:])
    assert all(np.array_equal(a, b) for a, b in zip(tn[1:3], tn3[:2])) and tuple(tn[3:]) == tuple(tn3[2:])
    # any two of the three
    for others in ((m.evidence_begin, (32, 0), m.evidence_end), (m.tone_begin, (8, 8, 255), m.tone_end)):
        others[0](*others[1])
        try:
            assert _same(_session(m, S0, lambda: m.match_frames(frames)), sync)
        finally:
            others[2]()


def test_a_unit_that_is_run_again_counts_once(capi, monkeypatch, cfg0, cfg0_data):
    """A matcher that starts with 512 pre-drawn RNG outputs.  Through the features tap: H1's five votes on one line sample far past
    them, the tap's loop runs its rows again.  Through match_frames and submit / collect: cfg0's candidates without a model do the
    same, and unit_collect runs the unit again from its frames.  The stream's length shows that the re-run happened; the sums equal
    a default matcher's."""
    case = VC.build(VC.h1, (1,))
    cfg = small_cfg(capi, **case.cfg)
    frames, kps, descs = _inputs(case)
    s = (16, 0, P.REACHES[0])
    m = _features_matcher(capi, case, cfg)
    want = _session(m, s, lambda: m.match_features(frames, kps, descs))
    m.close()
    monkeypatch.setenv("SLIDEO_RNG_STREAM_LEN", "512")
    m = _features_matcher(capi, case, cfg)
    assert m.rng_stream_len() == 512
    got = _session(m, s, lambda: m.match_features(frames, kps, descs))
    grown = m.rng_stream_len()
    assert grown > 512                                                             # the unit was run again
    again = _session(m, s, lambda: m.match_features(frames, kps, descs))           # (the stream has grown: no re-run now)
    assert m.rng_stream_len() == grown
    m.close()
    assert want[3] == 1 and want[1][0].any()
    assert got[0].tobytes() == want[0].tobytes() and _same(got, want) and _same(again, want)
    import torch
    _, cfg, frames, plain, sync = cfg0
    pages = cfg0_data[0]
    t = torch.from_numpy(frames).cuda()
    for path in ("sync", "submit"):
        m = capi.Matcher(cfg)
        m.add_pages(list(pages)); m.finalize()
        assert m.rng_stream_len() == 512
        if path == "sync":
            got = _session(m, S0, lambda: m.match_frames(frames))
        else:
            got = _session(m, S0, lambda: m.collect(m.submit_dev(t.data_ptr(), len(frames), W, H)))
        assert m.rng_stream_len() > 512, path                                      # the unit was run again
        assert got[0].tobytes() == plain.tobytes() and _same(got, sync), path
        m.close()
    monkeypatch.delenv("SLIDEO_RNG_STREAM_LEN")


def test_frames_limit(capi, cfg0, monkeypatch):
    """The refusal of a call that could take the frames through past the session's limit, with the limit lowered to 10 frames
    (SLIDEO_PLACEMENT_MAX_FRAMES, read at begin): the frames through, those of units in flight and the call's own all count."""
    import torch
    m, cfg, frames, plain, sync = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    monkeypatch.setenv("SLIDEO_PLACEMENT_MAX_FRAMES", "10")
    m.placement_begin(*S0)
    monkeypatch.delenv("SLIDEO_PLACEMENT_MAX_FRAMES")
    assert code(lambda: m.match_frames(np.concatenate([frames, frames[:3]]))) == 1     # 11 frames at once
    assert m.placement_info()["aw"] == 0                                               # (refused before anything ran)
    m.match_frames(frames)                                                             # 8 through
    assert m.placement_info()["frames_through"] == 8
    assert code(lambda: m.match_frames(frames[:3])) == 1                               # 8 + 3 = 11
    m.match_frames(frames[:2])                                                         # 10: the limit itself is allowed
    t = torch.from_numpy(frames).cuda()
    m.placement_end()
    monkeypatch.setenv("SLIDEO_PLACEMENT_MAX_FRAMES", "10")
    m.placement_begin(*S0)
    monkeypatch.delenv("SLIDEO_PLACEMENT_MAX_FRAMES")
    a = m.submit_dev(t.data_ptr(), 4, W, H)
    b = m.submit_dev(t.data_ptr(), 4, W, H)                                            # 4 in flight + 4
    with pytest.raises(capi.SlideoError) as e:                                         # 8 in flight + 3
        m.submit_dev(t.data_ptr(), 3, W, H)
    assert e.value.code == 1 and "11 frames" in str(e.value)
    m.collect(a); m.collect(b)
    assert m.placement_info()["frames_through"] == 8
    m.placement_end()
    m.placement_begin(*S0)                                                             # the default limit again
    m.match_frames(np.concatenate([frames, frames[:3]]))
    m.placement_end()


def test_rules(capi, cfg0):
    import torch
    m, cfg, frames, plain, sync = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    for cell in (0, 8, 24, 128, -16):
        assert code(lambda: m.placement_begin(cell, 0, 3.0)) == 1
    assert code(lambda: m.placement_begin(32, -1, 3.0)) == 1
    for reach in (0.0, -1.0, float("nan"), float("inf"), 1e200):
        assert code(lambda: m.placement_begin(32, 0, reach)) == 1
    assert code(m.placement_info) == 4 and code(m.placement_sums) == 4                # the state "none"
    m.placement_end()                                                                 # (fine in the state "none")
    m.placement_begin(32, 0, 0.5)
    assert code(lambda: m.placement_begin(16, 0, 3.0)) == 4                           # a session is open
    i = m.placement_info()
    assert (i["cell"], i["reach"], i["aw"], i["gw"], i["frames_through"]) == (32, 0.5, 0, 0, 0)
    sums, through, counted = m.placement_sums()
    assert sums.shape == (5, 0, 0) and (through, counted) == (0, 0)                   # nothing counted after begin
    m.match_frames(frames[:3])
    a = m.placement_sums()
    assert a[0].shape == (5, 12, 20) and a[0][0].any() and a[1] == 3
    with pytest.raises(capi.SlideoError) as e:                                        # another analysed size: both sizes named
        m.match_frames(np.zeros((1, 180, 320, 3), np.uint8))
    assert e.value.code == 1 and "320x180" in str(e.value) and "640x360" in str(e.value)
    b = m.placement_sums()
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    m.placement_end()
    m.placement_begin(32, 0, 0.5)                                                     # a new session starts from zero
    m.match_frames(frames[:3])
    b = m.placement_sums()
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    # a setter that changes the analysed image ends the session; a mask change does not
    m.set_frame_mask(np.full((H, W), 255, np.uint8))
    assert m.placement_info()["frames_through"] == 3
    m.set_frame_mask(None)
    m.set_working_size(0, 0)
    assert code(m.placement_info) == 4
    # units in flight: no begin
    t = torch.from_numpy(frames).cuda()
    ticket = m.submit_dev(t.data_ptr(), 2, W, H)
    assert code(lambda: m.placement_begin(32, 0, 3.0)) == 4
    m.collect(ticket)
    # SIFT mode, either order
    s = capi.Matcher(small_cfg(capi))
    s.placement_begin(32, 0, 3.0)
    assert code(lambda: s.use_sift(capi.sift_config(), 0.75)) == 5
    s.placement_end()
    s.use_sift(capi.sift_config(), 0.75)
    assert code(lambda: s.placement_begin(32, 0, 3.0)) == 5
    s.close()


@pytest.fixture(scope="module")
def use_scene(capi, synth):
    pages, frames, truth = P.keystone_scene(synth)
    U = P.USE
    m = capi.Matcher(small_cfg(capi, nfeatures=U["nfeatures"], min_rating=U["min_rating"]))
    m.add_pages(list(pages)); m.finalize()
    yield m, frames, truth
    m.close()


def _learn(matching, m, batches, **over):
    U = P.USE
    kw = dict(cell=U["cell"], min_inliers=U["min_inliers"], reach=U["reach"], min_count=U["min_count"], trim=U["trim"], rounds=U["rounds"])
    kw.update(over)
    return matching.learn_frame_quad_from_matches(m, batches, **kw)


def test_the_use(capi, use_scene):
    """The keystone scene (tests/placement_ref.py keystone_scene).  The learnt quad is within USE["bound_px"] of the scene's quad at
    every corner (the bound test_placement_abi.py test_the_use_on_the_cpu records); with the learnt region set, the share of frames
    assigned to the truth and the mean winning inliers are not lower than without."""
    from slideo_amd import matching
    m, frames, truth = use_scene
    U = P.USE
    batches = [frames[:len(frames) // 2], frames[len(frames) // 2:]]
    before = m.match_frames(frames)
    sw, sh, quad, ow, oh = _learn(matching, m, batches)
    assert pytest.raises(capi.SlideoError, m.placement_info).value.code == 4          # the learner ends its session
    err = P.corner_error(quad)
    assert (sw, sh) == (E.CANVAS_W, E.CANVAS_H)
    q = np.array(quad)
    d = lambda a, b: float(np.hypot(*(q[a] - q[b])))
    assert (ow, oh) == (int(round((d(0, 1) + d(3, 2)) / 2)), int(round((d(0, 3) + d(1, 2)) / 2)))
    # the learner's quad is what the session's sums give
    _, sums, through, counted = _session(m, (U["cell"], U["min_inliers"], U["reach"]), lambda: m.match_frames(frames))
    want = P.quad(sums, U["cell"], E.CANVAS_W, E.CANVAS_H, U["min_count"], U["trim"], U["rounds"], guard=False)
    assert want is not None and np.abs(q - want[0]).max() <= 1e-3
    m.set_frame_region(sw, sh, quad, ow, oh)
    try:
        after = m.match_frames(frames)
    finally:
        m.clear_frame_region()
    right0, right1 = float((before["page_idx"] == truth).mean()), float((after["page_idx"] == truth).mean())
    print("the use: %d of %d frames contribute; largest corner error %.2f px (bound %.0f); region %dx%d; right %.3f without and %.3f with the "
          "learnt region; mean winning inliers %.2f and %.2f" % (counted, through, err, U["bound_px"], ow, oh, right0, right1,
                                                                 before["inliers"].mean(), after["inliers"].mean()))
    assert err <= U["bound_px"]
    assert right1 >= right0 and after["inliers"].mean() >= before["inliers"].mean()
    # inset and out_size
    inset = _learn(matching, m, batches, inset=8, out_size=(320, 180))
    qi = np.array(inset[2])
    assert inset[3:] == (320, 180) and qi[0, 0] > q[0, 0] and qi[0, 1] > q[0, 1] and qi[2, 0] < q[2, 0] and qi[2, 1] < q[2, 1]
    assert 7.0 < float(np.hypot(*(qi[0] - q[0]))) < 13.0


def test_learner_refusals(capi, use_scene):
    from slideo_amd import matching
    m, frames, truth = use_scene
    with pytest.raises(capi.SlideoError):                                             # no cell holds that many keypoints
        _learn(matching, m, [frames[:2]], min_count=10 ** 6)
    with pytest.raises(ValueError, match="negative"):
        _learn(matching, m, [frames[:2]], inset=-1)
    with pytest.raises(ValueError, match="no frame was matched"):
        _learn(matching, m, [])
    with pytest.raises(ValueError, match="leaves nothing"):
        _learn(matching, m, [frames[:4]], inset=400)
    m.set_working_size(480, 270)
    try:
        with pytest.raises(ValueError, match="960x540 but were analysed at 480x270"):
            _learn(matching, m, [frames[:2]])
    finally:
        m.set_working_size(0, 0)
    assert pytest.raises(capi.SlideoError, m.placement_info).value.code == 4          # a failed learner leaves no session open
