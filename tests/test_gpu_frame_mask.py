"""Frame detection mask (include/slideo_amd.h "Frame mask") on the GPU: the mask pyramid against the CPU resize, the candidate
filter against its definition restated in numpy over an unbounded (all-keypoints) ORB run, and the frame paths against each other.
Masks hold only 0 and 255."""
import numpy as np
import pytest

import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

ALL_KP = 1 << 20            # an nfeatures no level's candidate count reaches (asserted where it is used)
HOLE = (100, 260, 200, 440)  # rows, columns of the hole in the 640x360 frames' mask: across the middle of the slide


def _levels(oracle, mask, cfg):
    """The mask pyramid of the header, on the CPU: resize_linear_exact level by level, then v > 254 ? v : 0."""
    h, w = mask.shape
    ws, hs, sc = oracle.pyramid_sizes(w, h, cfg)
    out = [np.ascontiguousarray(mask)]
    for l in range(1, cfg.nlevels):
        r = oracle.resize_linear_exact(out[-1], int(ws[l]), int(hs[l]))
        out.append(np.where(r > 254, r, 0).astype(np.uint8))
    return out, sc


def _rect_hole(h, w, y0, y1, x0, x1):
    m = np.full((h, w), 255, np.uint8)
    m[y0:y1, x0:x1] = 0
    return m


@pytest.fixture(scope="module")
def m500(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


@pytest.fixture(scope="module")
def mall(capi):
    m = capi.Matcher(small_cfg(capi, nfeatures=ALL_KP))
    yield m
    m.close()


@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    """cfg0's pages in a finalized matcher, a mask with a rectangle hole, and the masked host BGR call: verdicts and traces."""
    pages, frames, truth, _ = cfg0_data
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    plain = m.match_frames(frames)
    mask = _rect_hole(360, 640, *HOLE)
    m.set_frame_mask(mask)
    ref = m.match_frames(frames)
    traces = [m.last_candidates(i) for i in range(len(frames))]
    assert (ref["n_keypoints"] != plain["n_keypoints"]).any()          # the mask bears on these frames
    yield m, mask, ref, traces
    m.close()


def _same_traces(m, traces, what, idx=None):
    for k, i in enumerate(range(len(traces)) if idx is None else idx):
        got = m.last_candidates(k)
        assert got.tobytes() == traces[i].tobytes(), "%s: trace of frame %d" % (what, i)


# ---- 1. the mask pyramid -------------------------------------------------------------------------------------------------------

def _pyramid_masks(h, w):
    rng = np.random.default_rng(h * 4099 + w)
    single = np.full((h, w), 255, np.uint8)
    single[rng.integers(0, h, 40), rng.integers(0, w, 40)] = 0
    single[0, 0] = single[h - 1, w - 1] = single[0, w - 1] = 0
    yy, xx = np.mgrid[0:h, 0:w]
    return {"rect": _rect_hole(h, w, h // 3 + 1, h - 7, w // 5 + 2, w - 13), "single": single,
            "checker": (((yy + xx) & 1) * 255).astype(np.uint8), "all255": np.full((h, w), 255, np.uint8),
            "all0": np.zeros((h, w), np.uint8)}


@pytest.mark.parametrize("h,w,cases", [(360, 640, None), (203, 317, None), (130, 140, None), (1080, 1920, ("rect", "single"))])
def test_mask_pyramid_is_the_image_pyramids_resize_then_threshold(capi, oracle, m500, h, w, cases):
    oc = small_cfg(oracle)
    for name, mask in _pyramid_masks(h, w).items():
        if cases and name not in cases:
            continue
        m500.set_frame_mask(mask)
        assert m500.frame_mask_info == (w, h)
        want, _ = _levels(oracle, mask, oc)
        for l in range(oc.nlevels):
            got = m500.frame_mask_level(l)
            assert got.shape == want[l].shape, (name, l)
            assert np.array_equal(got, want[l]), "%s %dx%d level %d: %d px differ" % (name, w, h, l, (got != want[l]).sum())
            assert set(np.unique(got)) <= {0, 255}
            # 640x360: no output row of level 1 sits on a source row (its y centres are 0.1, 0.3, ... past one), so every value
            # there mixes a 0 with a 255 and nothing survives the threshold; deeper levels resize zeros
            if name == "checker" and l > 0 and (h, w) == (360, 640):
                assert not got.any()
            if name == "all255":
                assert got.all()
    m500.set_frame_mask(None)
    assert m500.frame_mask_info is None


# ---- 2. the filter's definition ------------------------------------------------------------------------------------------------

def _filter_cases(cfg0_data, synth):
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (360, 640, 3), dtype=np.uint8)
    top = np.zeros((360, 640), np.uint8)
    top[:100] = 255                                                   # deep levels' keep-regions start below the strip: emptied
    odd = (rng.integers(0, 256, (203, 317, 3), dtype=np.uint8) // 64 * 64).astype(np.uint8)
    tiny = rng.integers(0, 256, (130, 140, 3), dtype=np.uint8)
    pages = synth.pages(1)
    big, _, _ = synth.frames(pages, 1, first=2)
    return [("noise-top-strip", noise, top),
            ("frame-inset", cfg0_data[1][3], _rect_hole(360, 640, *HOLE)),
            ("odd-last-tile", odd, _rect_hole(203, 317, 110, 203, 180, 317)),       # crosses the keep-region's last tile column and last rows
            ("tiny", tiny, _rect_hole(130, 140, 60, 75, 40, 100)),
            ("1080p", big[0], _rect_hole(1080, 1920, 700, 1080, 1400, 1920))]


def test_filter_equals_its_definition_over_an_unbounded_run(capi, oracle, m500, mall, cfg0_data, synth):
    oc = small_cfg(oracle)
    quota = oracle.level_quotas(oc)
    quota_all = oracle.level_quotas(small_cfg(oracle, nfeatures=ALL_KP))
    seen = {"binds": 0, "free": 0, "emptied": 0, "lt256": 0, "gt256": 0, "ragged": 0}
    for name, img, mask in _filter_cases(cfg0_data, synth):
        h, w = mask.shape
        levels, sc = _levels(oracle, mask, oc)
        mall.set_frame_mask(None)
        kp, desc = mall.orb(img, cap=1 << 16)                        # every candidate FAST + NMS leaves, in canonical order
        octv = kp["octave"]
        cnt_all = np.bincount(octv, minlength=oc.nlevels)
        assert (cnt_all < quota_all).all(), (name, cnt_all, quota_all)        # the run is unbounded on every level
        xl = np.rint(kp["x"] / sc[octv]).astype(np.int64)
        yl = np.rint(kp["y"] / sc[octv]).astype(np.int64)
        assert np.array_equal(xl.astype(np.float32) * sc[octv], kp["x"]) and np.array_equal(yl.astype(np.float32) * sc[octv], kp["y"])
        alive = np.zeros(len(kp), bool)
        for l in range(oc.nlevels):
            s = octv == l
            alive[s] = levels[l][yl[s], xl[s]] != 0
        keep = alive.copy()
        for l in range(oc.nlevels):                                   # retainBest(quota): the n-th best response, ties kept
            s = alive & (octv == l)
            n_l, c = int(s.sum()), int(cnt_all[l])
            if n_l > quota[l]:
                thr = np.sort(kp["response"][s])[::-1][quota[l] - 1] if quota[l] > 0 else np.inf
                keep &= ~s | (kp["response"] >= thr)
                seen["binds"] += 1
            elif n_l > 0:
                seen["free"] += 1
            elif c > 0:
                seen["emptied"] += 1
            seen["lt256"] += 0 < c < 256
            seen["gt256"] += c > 256
            seen["ragged"] += c > 256 and c % 256 != 0
        m500.set_frame_mask(mask)
        gk, gd = m500.orb(img)
        assert len(gk) == keep.sum(), "%s: %d keypoints, the definition keeps %d" % (name, len(gk), keep.sum())
        assert gk.tobytes() == kp[keep].tobytes(), name
        assert np.array_equal(gd, desc[keep]), name
        # the same image at the mask's size in a matcher without a mask, and at another size under the mask: unmasked
        if name == "frame-inset":
            m500.set_frame_mask(None)
            plain = m500.orb(img)
            m500.set_frame_mask(np.zeros((40, 50), np.uint8))
            other = m500.orb(img)
            assert plain[0].tobytes() == other[0].tobytes() and np.array_equal(plain[1], other[1])
            assert plain[0].tobytes() != gk.tobytes()                 # and the hole bears on this frame
    m500.set_frame_mask(None)
    assert all(v > 0 for v in seen.values()), seen


# ---- 3. all 255 and all 0 on the host BGR path ---------------------------------------------------------------------------------

def test_all_255_is_no_mask_and_all_0_finds_nothing(capi, cfg0_data):
    pages, frames, truth, _ = cfg0_data
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    ref = m.match_frames(frames)
    traces = [m.last_candidates(i) for i in range(len(frames))]
    assert list(ref["page_idx"]) == list(truth)
    m.set_frame_mask(np.full((360, 640), 255, np.uint8))
    got = m.match_frames(frames)
    assert got.tobytes() == ref.tobytes()
    _same_traces(m, traces, "all 255")
    m.set_frame_mask(np.zeros((360, 640), np.uint8))
    got = m.match_frames(frames)
    assert (got["n_keypoints"] == 0).all() and (got["page_idx"] == -1).all()
    assert len(m.orb(frames[0])[0]) == 0
    m.set_frame_mask(None)
    assert m.match_frames(frames).tobytes() == ref.tobytes()
    m.close()


# ---- 4. end to end uses exactly the tap's features -----------------------------------------------------------------------------

def test_end_to_end_votes_are_those_of_the_taps_features(capi, oracle, cfg0_data, deck):
    pages, frames, truth, _ = cfg0_data
    m, mask, ref, traces = deck
    cfg = small_cfg(capi)
    rows, row_page = [], []
    for p in range(len(pages)):
        _, d = m.page_features(p)
        rows.append(d); row_page.append(np.full(len(d), p))
    rows, row_page = np.concatenate(rows), np.concatenate(row_page)
    tol = np.float32(cfg.vote_tolerance)
    for i in (1, 3, 7):
        kp, desc = m.orb(frames[i])
        assert ref["n_keypoints"][i] == len(kp)
        inside = (kp["y"] >= HOLE[0]) & (kp["y"] < HOLE[1]) & (kp["x"] >= HOLE[2]) & (kp["x"] < HOLE[3])
        assert not ((kp["octave"] == 0) & inside).any()               # nothing detected inside the hole
        idx, dist = oracle.knn_hamming(desc, rows, cfg.knn_k)
        best = dist[:, 0].astype(np.float32)
        ok = (dist.astype(np.float32) < (best * tol)[:, None]) & (best > 0)[:, None] & (idx >= 0)
        votes = np.bincount(row_page[idx[ok]], minlength=len(pages))
        assert len(traces[i]) > 0
        for c in traces[i]:
            assert c["n_votes"] == votes[c["page_idx"]], (i, c["page_idx"], c["n_votes"], votes)
        assert votes.max() == traces[i]["n_votes"].max()


# ---- 5. every frame path agrees ------------------------------------------------------------------------------------------------

def test_device_and_streaming_paths(capi, cfg0_data, deck):
    import torch
    pages, frames, _, _ = cfg0_data
    m, mask, ref, traces = deck
    t = torch.from_numpy(frames).cuda()
    fb = 640 * 360 * 3
    assert m.match_frames_dev(t.data_ptr(), len(frames), 640, 360).tobytes() == ref.tobytes()
    _same_traces(m, traces, "device BGR")
    tk = [m.submit_dev(t.data_ptr(), 3, 640, 360), m.submit_dev(t.data_ptr() + 3 * fb, 4, 640, 360),
          m.submit_dev(t.data_ptr() + 7 * fb, 1, 640, 360)]
    got = np.concatenate([m.collect(x) for x in tk])
    assert got.tobytes() == ref.tobytes()
    _same_traces(m, traces, "submit / collect")


def test_nv12_equals_the_bgr_call_on_the_converted_image(capi, cfg0_data, deck):
    pages, frames, _, _ = cfg0_data
    m, mask, _, _ = deck
    L, fbytes = capi.yuv420_layout("nv12", 640, 360)
    yuv = yref.frames_to_yuv(frames[:4], L, fbytes)
    conv = np.stack([m.yuv420_to_bgr(y, 640, 360, L) for y in yuv])
    want = m.match_frames(conv)
    tr = [m.last_candidates(i) for i in range(4)]
    got = m.match_frames_yuv420(yuv, 640, 360, L)
    assert got.tobytes() == want.tobytes()
    _same_traces(m, tr, "nv12")
    assert (want["n_keypoints"] > 0).any()


def test_reduced_frames_take_the_mask_at_the_reduced_size(capi, cfg0_data, deck):
    pages, frames, _, _ = cfg0_data
    m, mask, ref, traces = deck
    big = np.ascontiguousarray(frames.repeat(2, axis=1).repeat(2, axis=2))      # its 2x2 INTER_AREA reduction is `frames` again
    assert np.array_equal(m.reduce(big[0], 640, 360), frames[0])
    with pytest.raises(capi.SlideoError) as e:                                  # analysed at 1280x720: not the mask's size
        m.match_frames(big)
    assert e.value.code == 1 and "1280x720" in str(e.value) and "640x360" in str(e.value)
    m.set_working_size(640, 360)
    try:
        assert m.match_frames(big).tobytes() == ref.tobytes()
        _same_traces(m, traces, "working size")
    finally:
        m.set_working_size(0, 0)


def test_gated_call_and_the_kept_frames_pair(capi, cfg0_data, deck):
    pages, frames, _, _ = cfg0_data
    m, mask, ref, traces = deck
    m.gate_reset(None)
    changed, sim, got = m.match_changed_frames(frames)
    assert changed[0] and changed.sum() >= 2
    idx = np.flatnonzero(changed)
    assert got[idx].tobytes() == ref[idx].tobytes()
    _same_traces(m, traces, "gated", idx)
    ch2, sim2, _ = m.changed_mask(frames)                      # the gate sees whole frames: the mask call's flags, mask or not
    assert np.array_equal(changed, ch2) and np.array_equal(sim, sim2)
    assert m.match_kept_frames(np.arange(len(frames))).tobytes() == ref.tobytes()
    _same_traces(m, traces, "kept frames")
    m.gate_reset(None)


def test_group_on_one_device_twice(capi, cfg0_data, deck):
    pages, frames, _, _ = cfg0_data
    m, mask, ref, traces = deck
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    g.set_frame_mask(mask)
    assert g.member(1).frame_mask_info == (640, 360)
    assert g.match_frames(frames).tobytes() == ref.tobytes()
    _same_traces(g, traces, "group")
    with pytest.raises(capi.SlideoError) as e:
        g.match_frames(frames[:, :200])
    assert e.value.code == 1
    g.set_frame_mask(None)
    assert g.member(0).frame_mask_info is None
    g.close()


def test_overflowed_unit_is_rerun_under_the_mask(capi, cfg0_data, monkeypatch):
    """Equal corners everywhere: every score ties, retainBest keeps them all, and the frame has more keypoints than the
    capacity-sized path provides for (max(2 nfeatures, nfeatures + 1024)): the unit is re-run through the exact-size path, which
    must filter again.  Held against the exact-size path from the start and against the tap."""
    pages = cfg0_data[0]
    nf = 40
    img = np.full((360, 640, 3), 255, np.uint8)
    for y in range(2, 354, 12):
        for x in range(2, 634, 12):
            img[y:y + 6, x:x + 6] = 0
    frames = np.stack([img, cfg0_data[1][0]])
    mask = _rect_hole(360, 640, 0, 360, 500, 640)
    out = []
    for async_submit in ("1", "0"):
        monkeypatch.setenv("SLIDEO_ASYNC_SUBMIT", async_submit)
        m = capi.Matcher(small_cfg(capi, nfeatures=nf))
        m.add_pages(list(pages)); m.finalize()
        plain = m.match_frames(frames)
        m.set_frame_mask(mask)
        v = m.match_frames(frames)
        kp, _ = m.orb(img)
        assert v["n_keypoints"][0] == len(kp) > max(2 * nf, nf + 1024), len(kp)
        assert not (kp["x"] >= 510).any() and plain["n_keypoints"][0] > len(kp)
        out.append((v, [m.last_candidates(i) for i in range(2)]))
        m.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for a, b in zip(out[0][1], out[1][1]):
        assert a.tobytes() == b.tobytes()


# ---- 6. pages are never masked -------------------------------------------------------------------------------------------------

def test_pages_of_the_masks_size_are_not_masked(capi, cfg0_data):
    pages = cfg0_data[0]
    a = capi.Matcher(small_cfg(capi))
    b = capi.Matcher(small_cfg(capi))
    b.set_frame_mask(_rect_hole(450, 800, 100, 450, 0, 700))
    for m in (a, b):
        m.add_pages(list(pages[:2])); m.finalize()
    for p in range(2):
        (ka, da), (kb, db) = a.page_features(p), b.page_features(p)
        assert len(ka) > 100 and ka.tobytes() == kb.tobytes() and np.array_equal(da, db)
    assert len(b.orb(pages[0])[0]) < len(a.page_features(0)[0]) == len(a.orb(pages[0])[0])                  # (the tap, unlike the page calls, analyses a frame of that size)
    a.close(); b.close()


# ---- 7. errors and lifetime ----------------------------------------------------------------------------------------------------

def test_errors_and_lifetime(capi, oracle, cfg0_data):
    import torch
    pages, frames, _, _ = cfg0_data
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    with pytest.raises(capi.SlideoError) as e:                 # no mask: no level
        m.frame_mask_level(0)
    assert e.value.code == 4
    m.set_frame_mask(np.full((200, 300), 255, np.uint8))
    with pytest.raises(capi.SlideoError) as e:                 # size mismatch, both sizes named; not silently unmasked
        m.match_frames(frames)
    assert e.value.code == 1 and "640x360" in str(e.value) and "300x200" in str(e.value)
    with pytest.raises(capi.SlideoError) as e:
        m.frame_mask_level(8)
    assert e.value.code == 1
    L = capi.lib()
    buf = np.full((4, 4), 255, np.uint8)
    assert L.slideo_matcher_set_frame_mask(m._h, buf.ctypes.data, 0, 4, 4) == 1
    assert L.slideo_matcher_set_frame_mask(m._h, buf.ctypes.data, 4, 4, 3) == 1
    assert L.slideo_matcher_set_frame_mask(m._h, buf.ctypes.data, 5000, 4, 5000) == 5
    assert m.frame_mask_info == (300, 200)                      # refused calls leave the mask
    # a second mask replaces the pyramid
    second = _rect_hole(360, 640, 100, 200, 100, 300)
    m.set_frame_mask(second)
    want, _ = _levels(oracle, second, small_cfg(oracle))
    for l in (0, 3, 7):
        assert np.array_equal(m.frame_mask_level(l), want[l])
    masked = m.match_frames(frames)
    # a non-idle matcher
    t = torch.from_numpy(frames).cuda()
    tk = m.submit_dev(t.data_ptr(), 2, 640, 360)
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask(None)
    assert e.value.code == 4
    with pytest.raises(capi.SlideoError) as e:
        m.frame_mask_level(0)
    assert e.value.code == 4
    assert m.collect(tk).tobytes() == masked[:2].tobytes()
    # setting a mask ends the kept frames
    m.changed_mask(frames)
    m.set_frame_mask(second)
    with pytest.raises(capi.SlideoError) as e:
        m.match_kept_frames(np.arange(2))
    assert e.value.code == 4
    # NULL clears
    plain = capi.Matcher(small_cfg(capi))
    plain.add_pages(list(pages)); plain.finalize()
    m.set_frame_mask(None)
    assert m.frame_mask_info is None
    assert m.match_frames(frames).tobytes() == plain.match_frames(frames).tobytes()
    m.close(); plain.close()


def test_sift_mode_refuses_a_mask(capi):
    m = capi.Matcher(small_cfg(capi))
    m.use_sift(capi.sift_config())
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask(np.full((360, 640), 255, np.uint8))
    assert e.value.code == 5
    m.set_frame_mask(None)                                      # clearing nothing is not an error
    m.close()
    m = capi.Matcher(small_cfg(capi))
    m.set_frame_mask(np.full((360, 640), 255, np.uint8))
    with pytest.raises(capi.SlideoError) as e:
        m.use_sift(capi.sift_config())
    assert e.value.code == 5
    m.close()


# ---- 8. usefulness -------------------------------------------------------------------------------------------------------------

def inset_frame(frame, seed=3):
    """`frame` with a speaker-sized inset of random binary texture over a fifth of it (bottom right); the inset's rectangle."""
    h, w, _ = frame.shape
    ih, iw = int(round(h * 0.4472)), int(round(w * 0.4472))          # sqrt(0.2) of each side
    y0, x0 = h - ih, w - iw
    tex = np.random.default_rng(seed).integers(0, 2, (ih, iw), dtype=np.uint8) * 255
    out = frame.copy()
    out[y0:, x0:] = tex[:, :, None]
    return out, (y0, x0)


def test_masking_a_busy_inset_keeps_the_slide(capi, oracle, cfg0_data):
    pages, frames, truth, _ = cfg0_data
    i = int(np.flatnonzero(truth >= 0)[0])
    fr, (y0, x0) = inset_frame(frames[i])
    nf = None
    for cand in (500, 400, 300, 200, 150, 100):                  # the largest nfeatures at which the inset takes over half the keypoints
        kp, _ = oracle.orb(fr, small_cfg(oracle, nfeatures=cand))
        inside = (kp["x"] >= x0) & (kp["y"] >= y0)
        if inside.sum() * 2 > len(kp):
            nf = cand
            break
    assert nf is not None
    m = capi.Matcher(small_cfg(capi, nfeatures=nf))
    m.add_pages(list(pages)); m.finalize()
    plain = m.match_frames(fr[None])
    m.set_frame_mask(_rect_hole(fr.shape[0], fr.shape[1], y0, fr.shape[0], x0, fr.shape[1]))
    masked = m.match_frames(fr[None])
    print("nfeatures %d: unmasked page %d inliers %d, masked page %d inliers %d (truth %d)" %
          (nf, plain["page_idx"][0], plain["inliers"][0], masked["page_idx"][0], masked["inliers"][0], truth[i]))
    assert masked["page_idx"][0] == truth[i]
    assert masked["inliers"][0] >= plain["inliers"][0]
    m.close()
