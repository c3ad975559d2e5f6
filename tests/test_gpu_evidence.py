"""Match evidence map (include/slideo_amd.h "Match evidence map") on the GPU: evidence_kernel's counts against tests/evidence_ref.py
on constructed features (tests/verify_cases.py through Matcher.match_features) and on ORB's own (cfg0_data), the same counts from
every call form that runs the verify stage, no double counting when a unit is run again, and the session's rules."""
import numpy as np
import pytest

import evidence_ref as E
import verify_cases as VC
from conftest import small_cfg

pytestmark = pytest.mark.gpu

W, H = 640, 360


def _features_matcher(capi, case, cfg):
    m = capi.Matcher(cfg)
    smalls = {}
    for p in case.pages:
        if p.img not in smalls:
            smalls[p.img] = m.small_image(VC.page_image(p.img))
        m.add_page_features(VC.PAGE_W, VC.PAGE_H, VC.keypoints(p.xy), p.desc, smalls[p.img])
    m.finalize()
    return m


def _inputs(case):
    n = len(case.frames)
    return np.stack([case.frame_pixels(i) for i in range(n)]), [VC.keypoints(f.xy) for f in case.frames], [f.desc for f in case.frames]


def _session(m, cell, min_inliers, call):
    """(what `call` returns, seen, hit, frames_through, frames_counted) of one session around call()."""
    m.evidence_begin(cell, min_inliers)
    try:
        out = call()
        return (out,) + m.evidence_counts()
    finally:
        m.evidence_end()


@pytest.mark.parametrize("entry", E.constructed_cases(), ids=lambda e: e[0])
def test_counts_equal_restatement_on_constructed_features(capi, entry):
    """verify_model 0 and 1, the ratio test, several votes of a keypoint for the winner of which one passes (MULTI), frames without
    a verdict (X1; V1's empty frame), a frame below min_inliers (T2 at 22), a page set (V5 under deck pages 0, 7, 16), frames of
    more keypoints than the bitset's window (R2, H1), at cells 16, 32 and 64.  evidence_ref.counts asserts that no tested pair lies
    within 1e-9 relative of the threshold."""
    name, fa, pset, min_inliers = entry
    case = VC.build(*fa)
    cfg = small_cfg(capi, **case.cfg)
    m = _features_matcher(capi, case, cfg)
    train, tp, pxy = case.deck()
    rows = None
    if pset is not None:
        m.use_page_set(m.create_page_set(pset))
        rows = np.nonzero(np.isin(tp, pset))[0]
    frames, kps, descs = _inputs(case)
    plain = m.match_features(frames, kps, descs)
    for cell in (16, 32, 64):
        v, seen, hit, through, counted = _session(m, cell, min_inliers, lambda: m.match_features(frames, kps, descs))
        assert v.tobytes() == plain.tobytes()
        recs = [E.frame_record(cfg, f.xy, f.desc, v[i], m.last_candidates(i), train, rows) for i, f in enumerate(case.frames)]
        want = E.counts(recs, cell=cell, aw=W, ah=H, min_inliers=min_inliers, model=cfg.verify_model, thr=cfg.ransac_threshold,
                        train_page=tp, page_xy=pxy)
        print("%s cell %d: %d frames through, %d counted, %d seen, %d hit" % (name, cell, through, counted, seen.sum(), hit.sum()))
        assert (through, counted) == want[2:], name
        assert np.array_equal(seen, want[0]) and np.array_equal(hit, want[1]), (name, cell)
    if name in ("X1-none", "T2-below"):
        assert counted == 0 and not seen.any()
        assert name != "T2-below" or (v["page_idx"][0] >= 0 and v["inliers"][0] < min_inliers)
    elif name == "MULTI":
        assert counted == 1 and int(hit.sum()) == len(case.frames[0].xy) and sum(len(r["votes"]) for r in recs) == 2 * int(hit.sum())
    else:
        assert counted >= 1 and hit.any()
    if name == "V5-set":
        assert set(v["page_idx"]) <= set(pset)
    m.close()


@pytest.fixture(scope="module")
def cfg0(capi, cfg0_data):
    """The matcher of cfg0_data and the sync host call's session at cell 32 (computed once, shared, left unchanged)."""
    pages, frames, truth, _ = cfg0_data
    cfg = small_cfg(capi)
    m = capi.Matcher(cfg)
    m.add_pages(list(pages)); m.finalize()
    plain = m.match_frames(frames)
    sync = _session(m, 32, 0, lambda: m.match_frames(frames))
    yield m, cfg, frames, plain, sync
    m.close()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[1:3], b[1:3])) and tuple(a[3:]) == tuple(b[3:])


def test_sync_counts_equal_restatement_on_orb_features(capi, cfg0):
    m, cfg, frames, plain, sync = cfg0
    v, seen, hit, through, counted = sync
    assert v.tobytes() == plain.tobytes()                       # verdict bytes are identical with and without a session
    feats = [m.page_features(p) for p in range(m.page_count)]
    train = np.concatenate([d for _, d in feats])
    tp, pxy = E.deck_of(m, m.page_count)
    v2 = m.match_frames(frames)                                 # (the traces of the same call, outside the session)
    recs = []
    for i, f in enumerate(frames):
        kp, desc = m.orb(f)
        recs.append(E.frame_record(cfg, np.stack([kp["x"], kp["y"]], 1), desc, v2[i], m.last_candidates(i), train))
    want = E.counts(recs, cell=32, aw=W, ah=H, min_inliers=0, model=0, thr=cfg.ransac_threshold, train_page=tp, page_xy=pxy)
    print("cfg0: %d through, %d counted, %d seen, %d hit" % (through, counted, seen.sum(), hit.sum()))
    assert (through, counted) == want[2:] and counted >= 6
    assert np.array_equal(seen, want[0]) and np.array_equal(hit, want[1]) and hit.sum() > 100


def test_every_path_gives_the_same_counts(capi, cfg0, cfg0_data):
    import torch
    import yuv420_ref as Y
    m, cfg, frames, plain, sync = cfg0
    n = len(frames)
    fb = W * H * 3
    t = torch.from_numpy(frames).cuda()
    # a device call
    assert _same(_session(m, 32, 0, lambda: m.match_frames_dev(t.data_ptr(), n, W, H)), sync)
    # submit / collect with four units in flight on one accumulator
    def stream():
        tickets = [m.submit_dev(t.data_ptr() + 2 * i * fb, 2, W, H) for i in range(4)]
        assert m.evidence_info()["frames_through"] == 0         # (the frame counts are those of the collected units)
        with pytest.raises(capi.SlideoError) as e:
            m.evidence_counts()
        assert e.value.code == 4
        return np.concatenate([m.collect(x) for x in tickets])
    got = _session(m, 32, 0, stream)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    # kept frames of a mask call
    def kept():
        m.changed_mask(frames)
        return m.match_kept_frames(np.arange(n))
    got = _session(m, 32, 0, kept)
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    # a gated call: every frame twice, the second of each pair is unchanged and adds nothing
    def gated():
        m.gate_reset(None)
        ch, _, v = m.match_changed_frames(np.repeat(frames, 2, 0))
        assert list(ch) == [True, False] * n
        return v[::2]
    got = _session(m, 32, 0, gated)
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
        (ch, v), seen, hit, through, counted = _session(m, 32, 0, direct)
    finally:
        m.set_direct_similarity(0.0)
    is_direct = ch & (v["page_idx"] >= 0) & (v["inliers"] == 0) & (v["n_keypoints"] == 0)
    assert is_direct.any() and through == int((ch & ~is_direct).sum()) and 0 < through < len(seq)
    rest = seq[ch & ~is_direct]
    assert _same(((), seen, hit, through, counted), _session(m, 32, 0, lambda: m.match_frames(rest)))
    # one NV12 call: the counts of the BGR images the library makes of the frames
    L, nb = capi.yuv420_layout("nv12", W, H)
    yuv = Y.frames_to_yuv(frames, L, nb)
    bgr = np.stack([Y.to_bgr(f, W, H, L) for f in yuv])
    assert _same(_session(m, 32, 0, lambda: m.match_frames_yuv420(yuv, W, H, L)), _session(m, 32, 0, lambda: m.match_frames(bgr)))
    # a two-member group on device 0: the members' sums
    g = capi.Group(cfg, devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    got = _session(g, 32, 0, lambda: g.match_frames(frames))
    assert got[0].tobytes() == plain.tobytes() and _same(got, sync)
    g.close()


def test_a_unit_that_is_run_again_counts_once(capi, monkeypatch, cfg0, cfg0_data):
    """A matcher that starts with 512 pre-drawn RNG outputs (test_tap_grows_the_rng_stream_itself).  Through the features tap: H1's
    five votes on one line sample far past them, the tap's loop runs its rows again.  Through match_frames and submit / collect:
    cfg0's candidates without a model do the same, and unit_collect runs the unit again from its frames.  The stream's length shows
    that the re-run happened; the counts equal a default matcher's."""
    case = VC.build(VC.h1, (1,))
    cfg = small_cfg(capi, **case.cfg)
    frames, kps, descs = _inputs(case)
    m = _features_matcher(capi, case, cfg)
    want = _session(m, 16, 0, lambda: m.match_features(frames, kps, descs))
    m.close()
    monkeypatch.setenv("SLIDEO_RNG_STREAM_LEN", "512")
    m = _features_matcher(capi, case, cfg)
    assert m.rng_stream_len() == 512
    got = _session(m, 16, 0, lambda: m.match_features(frames, kps, descs))
    grown = m.rng_stream_len()
    assert grown > 512                                                             # the unit was run again
    again = _session(m, 16, 0, lambda: m.match_features(frames, kps, descs))       # (the stream has grown: no re-run now)
    assert m.rng_stream_len() == grown
    m.close()
    assert want[4] == 1 and want[2].any()
    assert got[0].tobytes() == want[0].tobytes() and _same(got, want) and _same(again, want)
    # unit_collect's re-run: a synchronous host call, then a submitted unit, each on a matcher with a fresh short stream
    import torch
    _, cfg, frames, plain, sync = cfg0
    pages = cfg0_data[0]
    t = torch.from_numpy(frames).cuda()
    for path in ("sync", "submit"):
        m = capi.Matcher(cfg)
        m.add_pages(list(pages)); m.finalize()
        assert m.rng_stream_len() == 512
        if path == "sync":
            got = _session(m, 32, 0, lambda: m.match_frames(frames))
        else:
            got = _session(m, 32, 0, lambda: m.collect(m.submit_dev(t.data_ptr(), len(frames), W, H)))
        assert m.rng_stream_len() > 512, path                                      # the unit was run again
        assert got[0].tobytes() == plain.tobytes() and _same(got, sync), path
        m.close()
    monkeypatch.delenv("SLIDEO_RNG_STREAM_LEN")


def test_frames_limit(capi, cfg0, monkeypatch):
    """The refusal of a call that could take frames_counted past the session's limit, with the limit lowered to 10 frames
    (SLIDEO_EVIDENCE_MAX_FRAMES, read at begin): counted frames, the frames of units in flight and the call's own all count."""
    import torch
    m, cfg, frames, plain, sync = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    monkeypatch.setenv("SLIDEO_EVIDENCE_MAX_FRAMES", "10")
    m.evidence_begin(32, 0)
    monkeypatch.delenv("SLIDEO_EVIDENCE_MAX_FRAMES")
    assert code(lambda: m.match_frames(np.concatenate([frames, frames[:3]]))) == 1     # 11 frames at once
    assert m.evidence_info()["aw"] == 0                                                # (refused before anything ran)
    m.match_frames(frames)
    counted = m.evidence_info()["frames_counted"]
    assert counted == sync[4] and counted <= 8
    assert code(lambda: m.match_frames(frames[:10 - counted + 1])) == 1                # counted + n = 11
    m.match_frames(frames[:1])                                                         # a frame without a verdict leaves room
    t = torch.from_numpy(frames).cuda()
    m.evidence_end()
    monkeypatch.setenv("SLIDEO_EVIDENCE_MAX_FRAMES", "10")
    m.evidence_begin(32, 0)
    monkeypatch.delenv("SLIDEO_EVIDENCE_MAX_FRAMES")
    a = m.submit_dev(t.data_ptr(), 4, W, H)
    b = m.submit_dev(t.data_ptr(), 4, W, H)                                            # 4 in flight + 4
    with pytest.raises(capi.SlideoError) as e:                                         # 8 in flight + 3
        m.submit_dev(t.data_ptr(), 3, W, H)
    assert e.value.code == 1 and "11 frames" in str(e.value)
    m.collect(a); m.collect(b)
    assert m.evidence_info()["frames_through"] == 8
    m.evidence_end()
    m.evidence_begin(32, 0)                                                            # the default limit again
    m.match_frames(np.concatenate([frames, frames[:3]]))
    m.evidence_end()


def test_rules(capi, cfg0):
    import torch
    m, cfg, frames, plain, sync = cfg0
    code = lambda fn: pytest.raises(capi.SlideoError, fn).value.code
    for cell in (0, 8, 24, 128, -16):
        assert code(lambda: m.evidence_begin(cell, 0)) == 1
    assert code(lambda: m.evidence_begin(32, -1)) == 1
    assert code(m.evidence_info) == 4 and code(m.evidence_counts) == 4                # the state "none"
    m.evidence_end()                                                                  # (fine in the state "none")
    m.evidence_begin(32, 0)
    assert code(lambda: m.evidence_begin(16, 0)) == 4                                 # a session is open
    i = m.evidence_info()
    assert (i["cell"], i["aw"], i["gw"], i["frames_through"], i["frames_counted"]) == (32, 0, 0, 0, 0)
    seen, hit, through, counted = m.evidence_counts()
    assert seen.size == 0 and hit.size == 0 and (through, counted) == (0, 0)          # nothing counted after begin
    m.match_frames(frames[:3])
    a = m.evidence_counts()
    assert a[0].shape == (12, 20) and a[0].any() and a[2] == 3
    with pytest.raises(capi.SlideoError) as e:                                        # another analysed size: both sizes named
        m.match_frames(np.zeros((1, 180, 320, 3), np.uint8))
    assert e.value.code == 1 and "320x180" in str(e.value) and "640x360" in str(e.value)
    b = m.evidence_counts()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    m.evidence_end()
    m.evidence_begin(32, 0)                                                           # a new session starts from zero
    m.match_frames(frames[:3])
    b = m.evidence_counts()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    # a setter that changes the analysed image ends the session; a mask change does not
    m.set_frame_mask(np.full((H, W), 255, np.uint8))
    assert m.evidence_info()["frames_through"] == 3
    m.set_frame_mask(None)
    m.set_working_size(0, 0)
    assert code(m.evidence_info) == 4
    # units in flight: no begin
    t = torch.from_numpy(frames).cuda()
    ticket = m.submit_dev(t.data_ptr(), 2, W, H)
    assert code(lambda: m.evidence_begin(32, 0)) == 4
    m.collect(ticket)
    # SIFT mode, either order
    s = capi.Matcher(small_cfg(capi))
    s.evidence_begin(32, 0)
    assert code(lambda: s.use_sift(capi.sift_config(), 0.75)) == 5
    s.evidence_end()
    s.use_sift(capi.sift_config(), 0.75)
    assert code(lambda: s.evidence_begin(32, 0)) == 5
    s.close()


@pytest.fixture(scope="module")
def use_scene(capi, synth):
    pages, frames, truth = E.canvas_scene(synth)
    m = capi.Matcher(small_cfg(capi, nfeatures=E.SCENE["nfeatures"]))
    m.add_pages(list(pages)); m.finalize()
    yield m, frames, truth
    m.close()


def test_the_use(capi, use_scene):
    """The canvas scene (tests/evidence_ref.py canvas_scene): a 640x360 window of cropped synth frames at a fixed offset in a
    960x540 canvas of static random texture.  The learnt box contains the window and exceeds it by less than a cell per side; the
    learnt mask keeps every cell wholly inside the window and zeroes at least half of the wholly-outside cells with seen >=
    min_seen; with the mask set the mean winning inliers over the batch are not lower than without.  Through the two learners of
    slideo_amd.matching, whose results must be what the session's counts give."""
    from slideo_amd import matching
    m, frames, truth = use_scene
    S = E.SCENE
    batches = [frames[:len(frames) // 2], frames[len(frames) // 2:]]
    before = m.match_frames(frames)
    assert (before["page_idx"] == truth).mean() >= 0.75
    mask = matching.learn_frame_mask_from_matches(m, batches, cell=S["cell"], min_inliers=S["min_inliers"], min_seen=S["min_seen"],
                                                  min_hit=S["min_hit"], grow=S["grow"])
    sw, sh, quad, ow, oh = matching.learn_frame_box_from_matches(m, batches, cell=S["cell"], min_inliers=S["min_inliers"],
                                                                 min_hits=S["min_hits"], min_hit=S["box_min_hit"])
    assert pytest.raises(capi.SlideoError, m.evidence_info).value.code == 4          # the learners end their sessions
    box = (int(quad[0][0]), int(quad[0][1]), int(quad[2][0]) + 1, int(quad[2][1]) + 1)
    assert (sw, sh) == (E.CANVAS_W, E.CANVAS_H) and (ow, oh) == (box[2] - box[0], box[3] - box[1])
    assert quad == [(box[0], box[1]), (box[2] - 1, box[1]), (box[2] - 1, box[3] - 1), (box[0], box[3] - 1)]
    _, seen, hit, through, counted = _session(m, S["cell"], S["min_inliers"], lambda: m.match_frames(frames))
    assert through == len(frames) and counted >= len(frames) // 2
    assert np.array_equal(mask, E.mask(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_seen"], int(S["min_hit"] * 1e6), S["grow"]))
    assert box == E.box(seen, hit, S["cell"], E.CANVAS_W, E.CANVAS_H, S["min_hits"], int(S["box_min_hit"] * 1e6))
    zeroed, outside = E.check_use(seen, hit, S["cell"], S["min_seen"], box, mask)
    inset = matching.learn_frame_box_from_matches(m, batches, cell=S["cell"], min_inliers=S["min_inliers"], min_hits=S["min_hits"],
                                                  min_hit=S["box_min_hit"], inset=5, out_size=(320, 180))
    assert inset[2][0] == (box[0] + 5, box[1] + 5) and inset[2][2] == (box[2] - 6, box[3] - 6) and inset[3:] == (320, 180)
    m.set_frame_mask(mask)
    try:
        after = m.match_frames(frames)
    finally:
        m.set_frame_mask(None)
    print("the use: box %s, %d of %d clutter cells zeroed, mean winning inliers %.2f without and %.2f with the mask, %d and %d right"
          % (box, zeroed, outside, before["inliers"].mean(), after["inliers"].mean(), (before["page_idx"] == truth).sum(),
             (after["page_idx"] == truth).sum()))
    assert after["inliers"].mean() >= before["inliers"].mean()


def test_learner_refusals(capi, use_scene):
    from slideo_amd import matching
    m, frames, truth = use_scene
    S = E.SCENE
    kw = dict(cell=S["cell"], min_inliers=S["min_inliers"], min_hits=S["min_hits"], min_hit=S["box_min_hit"])
    with pytest.raises(ValueError, match="empty or narrower"):                        # no cell holds that many hits
        matching.learn_frame_box_from_matches(m, [frames[:4]], **dict(kw, min_hits=10 ** 6))
    with pytest.raises(ValueError, match="negative"):
        matching.learn_frame_box_from_matches(m, [frames[:4]], inset=-1, **kw)
    with pytest.raises(ValueError, match="no frame was matched"):
        matching.learn_frame_mask_from_matches(m, [], cell=64, min_inliers=0, min_seen=1, min_hit=0.5, grow=0)
    m.set_working_size(480, 270)
    try:
        with pytest.raises(ValueError, match="960x540 but were analysed at 480x270"):
            matching.learn_frame_box_from_matches(m, [frames[:4]], **kw)
    finally:
        m.set_working_size(0, 0)
    assert pytest.raises(capi.SlideoError, m.evidence_info).value.code == 4          # a failed learner leaves no session open
