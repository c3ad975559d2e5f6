"""Page sets (include/slideo_amd.h "page sets"): frame calls made while a set S is selected return, bit for bit, what a reference
sub-matcher built from exactly S's pages returns (its page j mapped to the j-th smallest index of S) — verdicts and the full
candidate trace, on every frame path, under every search shape and option the exact Hamming search has."""
import os

import numpy as np
import pytest

from conftest import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deck48(synth):
    """48 pages of 800x450, 12 synthetic 640x360 frames showing some of them."""
    pages = synth.pages(48, 800, 450, seed=4242)
    frames, truth, _ = synth.frames(pages, 12, 640, 360, seed=77)
    return pages, frames, truth


def _matcher(capi, pages, **over):
    m = capi.Matcher(small_cfg(capi, **over))
    m.add_pages(list(pages))
    m.finalize()
    return m


def _sub_matcher(capi, m, S, **over):
    """The reference sub-matcher of set S: the same config, exactly S's pages in ascending deck order, imported from m."""
    sm = capi.Matcher(small_cfg(capi, **over))
    for p in sorted(S):
        kp, desc = m.page_features(p)
        small = m.page_small(p)
        sm.add_page_features(800, 450, kp, desc, small)
    sm.finalize()
    return sm


def _mapped(v, S):
    """A sub-matcher's records with its page indices mapped to deck indices."""
    S = np.array(sorted(S), np.int32)
    v = v.copy()
    v["page_idx"] = np.where(v["page_idx"] >= 0, S[np.maximum(v["page_idx"], 0)], v["page_idx"])
    return v


def _trace(m, n):
    return [m.last_candidates(i) for i in range(n)]


def _assert_same(v, t, vs, ts, S):
    assert v.tobytes() == _mapped(vs, S).tobytes(), (v, _mapped(vs, S))
    assert len(t) == len(ts)
    for a, b in zip(t, ts):
        assert a.tobytes() == _mapped(b, S).tobytes(), (a, _mapped(b, S))


def _check_set(capi, m, S, frames, sub=None, **over):
    """S selected on m: verdicts and traces equal the sub-matcher's."""
    sid = m.create_page_set(S)
    m.use_page_set(sid)
    v = m.match_frames(frames); t = _trace(m, len(frames))
    m.use_page_set(0)
    own = sub is None
    sub = sub or _sub_matcher(capi, m, S, **over)
    vs = sub.match_frames(frames); ts = _trace(sub, len(frames))
    _assert_same(v, t, vs, ts, S)
    m.release_page_set(sid)
    if own:
        sub.close()
    return v


def test_definition_against_the_sub_matcher(capi, deck48):
    pages, frames, truth = deck48
    m = _matcher(capi, pages)
    shown = sorted(set(int(p) for p in truth if p >= 0))
    assert shown, truth
    sets = {
        "every third": list(range(0, 48, 3)),
        "the frames' pages": shown + [p for p in (5, 17, 40) if p not in shown],
        "none of them": [p for p in range(48) if p not in shown][:10],
        "single": [shown[0]],
    }
    for name, S in sets.items():
        v = _check_set(capi, m, S[::-1], frames)          # (any order)
        assert all(p in S or p == -1 for p in v["page_idx"]), name
        if name == "the frames' pages":
            assert list(v["page_idx"]) == list(truth)
    # all pages: set 0 and the plain matcher
    v0 = m.match_frames(frames); t0 = _trace(m, len(frames))
    sid = m.create_page_set(range(48))
    info, deck = m.page_set_info(sid), m.page_set_info(0)
    assert (info["n_pages"], info["rows"], info["unique_rows"]) == (deck["n_pages"], deck["rows"], deck["unique_rows"]) == \
        (48, m.descriptor_count, m.unique_descriptor_count)
    m.use_page_set(sid)
    va = m.match_frames(frames); ta = _trace(m, len(frames))
    assert va.tobytes() == v0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(ta, t0))
    m.use_page_set(0); m.release_page_set(sid)
    plain = _matcher(capi, pages)
    assert plain.match_frames(frames).tobytes() == v0.tobytes()
    m.close(); plain.close()


def _dup_deck(capi, m):
    """A 52-page deck from m's 48 pages: pages 48..51 repeat pages 3, 7, 7 and 20 (every row of them duplicated across pages), and
    page 50 also carries half of page 11's rows."""
    d = capi.Matcher(small_cfg(capi))
    feats = [m.page_features(p) for p in range(48)]
    smalls = [m.page_small(p) for p in range(48)]
    for p in range(48):
        d.add_page_features(800, 450, feats[p][0], feats[p][1], smalls[p])
    for src in (3, 7, 7, 20):
        kp, desc = feats[src]
        if d.page_count == 50:
            kp = np.concatenate([kp, feats[11][0][::2]]); desc = np.concatenate([desc, feats[11][1][::2]])
        d.add_page_features(800, 450, kp, desc, smalls[src])
    d.finalize()
    return d


def test_duplicates_split_by_the_set(capi, deck48):
    pages, frames, truth = deck48
    m = _matcher(capi, pages)
    d = _dup_deck(capi, m)
    assert d.unique_descriptor_count < d.descriptor_count
    sets = [[3, 7, 11, 20], [48, 49, 50, 51], [3, 49, 50, 11], [7, 50], list(range(0, 52, 2)), list(range(52))]
    descs = [d.page_features(p)[1] for p in range(52)]
    for S in sets:
        sid = d.create_page_set(S)
        rows = np.concatenate([descs[p] for p in S])
        info = d.page_set_info(sid)
        assert info["n_pages"] == len(S) and info["rows"] == len(rows)
        assert info["unique_rows"] == len(np.unique(rows.view(np.dtype((np.void, 32)))))
        assert info["bytes"] > 0
        d.release_page_set(sid)
        _check_set(capi, d, S, frames)
    m.close(); d.close()


def test_every_frame_path(capi, deck48):
    """Host BGR, device BGR, YUV 4:2:0 (host and device), submit / collect with units of different sets in flight, and
    changed_mask + match_kept_frames."""
    import torch
    pages, frames, truth = deck48
    m = _matcher(capi, pages)
    A, B = list(range(0, 48, 2)), sorted(set(int(p) for p in truth if p >= 0) | {1, 9})
    subs = {0: None}
    ids = {}
    for S in (A, B):
        ids[tuple(S)] = m.create_page_set(S)
        subs[ids[tuple(S)]] = (_sub_matcher(capi, m, S), S)
    n, h, w = len(frames), 360, 640
    d_frames = torch.from_numpy(frames).cuda()
    yuv = np.stack([_nv12(f) for f in frames])
    d_yuv = torch.from_numpy(yuv).cuda()
    torch.cuda.synchronize()
    for S in (A, B):
        sid = ids[tuple(S)]
        sub = subs[sid][0]
        m.use_page_set(sid)
        vs = sub.match_frames(frames); ts = _trace(sub, n)
        _assert_same(m.match_frames(frames), _trace(m, n), vs, ts, S)
        _assert_same(m.match_frames_dev(d_frames.data_ptr(), n, w, h), _trace(m, n), vs, ts, S)
        vy = sub.match_frames_yuv420(yuv, w, h, "nv12"); ty = _trace(sub, n)
        _assert_same(m.match_frames_yuv420(yuv, w, h, "nv12"), _trace(m, n), vy, ty, S)
        layout, fs = capi.yuv420_layout_packed("nv12", w, h), w * h * 3 // 2
        _assert_same(m.match_frames_yuv420_dev(d_yuv.data_ptr(), n, w, h, layout, fs), _trace(m, n), vy, ty, S)
        seq = np.stack([frames[0], frames[0], frames[1], frames[2], frames[2], frames[3]])
        c, _, _ = m.changed_mask(seq)
        cs, _, _ = sub.changed_mask(seq)
        assert list(c) == list(cs)
        sel = np.nonzero(c)[0]
        assert m.match_kept_frames(sel).tobytes() == _mapped(sub.match_kept_frames(sel), S).tobytes()
    # submit / collect: units of set A, the deck and set B interleaved in flight
    plain = _matcher(capi, pages)
    order = [ids[tuple(A)], 0, ids[tuple(B)], ids[tuple(A)]]
    chunks = [(0, 3), (3, 6), (6, 9), (9, 12)]
    tickets = []
    for sid, (lo, hi) in zip(order, chunks):
        m.use_page_set(sid)
        tickets.append(m.submit_dev(d_frames[lo:hi].data_ptr(), hi - lo, w, h))
    with pytest.raises(capi.SlideoError) as e:          # searched by an uncollected unit
        m.release_page_set(ids[tuple(B)])
    assert e.value.code == 4
    m.use_page_set(0)
    for sid, (lo, hi), tk in zip(order, chunks, tickets):
        v = m.collect(tk)
        if sid == 0:
            assert v.tobytes() == plain.match_frames(frames[lo:hi]).tobytes()
        else:
            sub, S = subs[sid]
            assert v.tobytes() == _mapped(sub.match_frames(frames[lo:hi]), S).tobytes()
    for sid in ids.values():
        m.release_page_set(sid)
        subs[sid][0].close()
    m.close(); plain.close()


def _nv12(bgr):
    """A plausible NV12 frame for a BGR frame (BT.601 studio range; any YUV input serves, both matchers see the same)."""
    b, g, r = [bgr[..., i].astype(np.float32) for i in range(3)]
    y = np.clip(16 + 0.257 * r + 0.504 * g + 0.098 * b, 0, 255)
    u = np.clip(128 - 0.148 * r - 0.291 * g + 0.439 * b, 0, 255)
    v = np.clip(128 + 0.439 * r - 0.368 * g - 0.071 * b, 0, 255)
    h, w = y.shape
    uv = np.empty((h // 2, w // 2, 2), np.float32)
    uv[..., 0] = u.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    uv[..., 1] = v.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    return np.concatenate([y.round().astype(np.uint8).ravel(), uv.round().astype(np.uint8).ravel()])


@pytest.mark.parametrize("opt", ["ratio_test", "verify_model", "exact_lists", "share0", "share1", "share4", "dedup0", "engine2"])
def test_options_and_search_shapes(capi, deck48, opt, monkeypatch):
    pages, frames, truth = deck48
    over, env = {}, {}
    if opt == "ratio_test":
        over = dict(ratio_test=0.8)
    elif opt == "verify_model":
        over = dict(verify_model=1)
    elif opt.startswith("share"):
        env = {"SLIDEO_KNN_SHARE": opt[5:]}
    elif opt == "dedup0":
        env = {"SLIDEO_KNN_DEDUP": "0"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _matcher(capi, pages, **over)
    if opt == "dedup0":
        assert m.unique_descriptor_count == m.descriptor_count
    S = sorted(set(int(p) for p in truth if p >= 0) | set(range(1, 48, 5)))
    sub = _sub_matcher(capi, m, S, **over)
    if opt == "exact_lists":
        m.set_knn_exact_lists(True); sub.set_knn_exact_lists(True)
    if opt == "engine2":
        m.set_knn_engine("mfma4"); sub.set_knn_engine("mfma4")
    sid = m.create_page_set(S)
    if opt == "dedup0":
        info = m.page_set_info(sid)
        assert info["unique_rows"] == info["rows"]
    m.use_page_set(sid)
    n = len(frames)
    if opt.startswith("share"):
        # units in flight together (the shared-chip block shapes): submit / collect, four units
        import torch
        d = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        tk = [m.submit_dev(d[i:i + 3].data_ptr(), 3, 640, 360) for i in range(0, n, 3)]
        v = np.concatenate([m.collect(t) for t in tk])
        assert v.tobytes() == _mapped(sub.match_frames(frames), S).tobytes()
    _assert_same(m.match_frames(frames), _trace(m, n), sub.match_frames(frames), _trace(sub, n), S)
    m.use_page_set(0); m.release_page_set(sid)
    m.close(); sub.close()


def test_headline_size_once(capi, synth):
    """500-page deck of 2001x1125 pages, 64 1080p frames, a 100-page set holding the frames' pages."""
    pages = synth.pages(500, threads=min(64, os.cpu_count() or 1))
    frames, truth, _ = synth.frames(pages[:250], 64, 1920, 1080, seed=99)
    m = capi.Matcher(capi.default_config())
    m.add_pages(list(pages))
    m.finalize()
    shown = set(int(p) for p in truth if p >= 0)
    S = sorted(shown | set([p for p in range(250, 500, 2)][:100 - len(shown)]))
    assert len(S) == 100
    sub = capi.Matcher(capi.default_config())
    for p in S:
        kp, desc = m.page_features(p)
        sub.add_page_features(2001, 1125, kp, desc, m.page_small(p))
    sub.finalize()
    sid = m.create_page_set(S)
    m.use_page_set(sid)
    n = len(frames)
    v = m.match_frames(frames); t = _trace(m, n)
    _assert_same(v, t, sub.match_frames(frames), _trace(sub, n), S)
    m.close(); sub.close()


def test_no_leak_into_set_zero(capi, deck48):
    pages, frames, _ = deck48
    m = _matcher(capi, pages)
    for S in ([1, 2, 3], list(range(0, 48, 4)), [40]):
        sid = m.create_page_set(S)
        m.use_page_set(sid)
        m.match_frames(frames)
        m.use_page_set(0)
        m.release_page_set(sid)
    keep = m.create_page_set([5, 6])           # (a live set that is not selected)
    fresh = _matcher(capi, pages)
    n = len(frames)
    v = m.match_frames(frames); t = _trace(m, n)
    vf = fresh.match_frames(frames); tf = _trace(fresh, n)
    assert v.tobytes() == vf.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(t, tf))
    m.release_page_set(keep)
    m.close(); fresh.close()


def test_group_under_a_set(capi, deck48):
    pages, frames, truth = deck48
    m = _matcher(capi, pages)
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    S = list(range(0, 48, 3)) + [p for p in sorted(set(int(p) for p in truth if p >= 0)) if p % 3]
    sid, gid = m.create_page_set(S), g.create_page_set(S)
    assert gid >= 1 and all(g.member(r).page_set_info(gid) == m.page_set_info(sid) for r in range(2))
    m.use_page_set(sid); g.use_page_set(gid)
    n = len(frames)
    v = m.match_frames(frames); t = _trace(m, n)
    assert g.match_frames(frames).tobytes() == v.tobytes()
    assert all(g.last_candidates(i).tobytes() == t[i].tobytes() for i in range(n))
    with pytest.raises(capi.SlideoError) as e:
        g.release_page_set(gid)                  # selected
    assert e.value.code == 4
    g.use_page_set(0); g.release_page_set(gid)
    with pytest.raises(capi.SlideoError) as e:
        g.use_page_set(gid)
    assert e.value.code == 1
    m.close(); g.close()


def test_errors(capi, deck48, synth):
    pages, frames, _ = deck48
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages[:6]))
    for call in (lambda: m.create_page_set([0]), lambda: m.use_page_set(0), lambda: m.page_set_info(0)):
        with pytest.raises(capi.SlideoError) as e:              # before finalize
            call()
        assert e.value.code == 4
    blank = np.full((450, 800, 3), 255, np.uint8)              # a page without a single keypoint
    m.add_pages([blank])
    m.finalize()
    assert m.page_features(6)[0].shape[0] == 0

    def code(fn):
        with pytest.raises(capi.SlideoError) as e:
            fn()
        return e.value.code
    assert code(lambda: m.create_page_set([])) == 1
    assert code(lambda: m.create_page_set([0, 0])) == 1
    assert code(lambda: m.create_page_set([7])) == 1           # out of range (the library's check)
    assert code(lambda: m.use_page_set(5)) == 1                # unknown
    assert code(lambda: m.release_page_set(0)) == 1
    assert code(lambda: m.page_set_info(9)) == 1
    assert code(lambda: m.create_page_set([6])) == 6           # no descriptor
    sid = m.create_page_set([1, 6])
    m.use_page_set(sid)
    assert code(lambda: m.release_page_set(sid)) == 4          # selected
    m.set_knn_engine("valu")                                   # VALU engine: refused at the first frame call ...
    assert code(lambda: m.match_frames(frames[:2])) == 5
    m.use_page_set(0)
    assert code(lambda: m.use_page_set(sid)) == 5              # ... and at use_page_set
    m.set_knn_engine("mfma")
    m.release_page_set(sid)
    live = [m.create_page_set([i % 6]) for i in range(64)]
    assert code(lambda: m.create_page_set([0])) == 5            # 65 live sets
    for s in live:
        m.release_page_set(s)
    m.create_page_set([0])
    m.close()
    # LSH and SIFT matchers
    lsh = _matcher(capi, pages[:4], matcher=1)
    assert code(lambda: lsh.create_page_set([0, 1])) == 5
    lsh.close()
    sm = capi.Matcher(small_cfg(capi))
    sm.use_sift(capi.sift_config(nfeatures=300), 0.0)
    sm.add_pages(list(pages[:4])); sm.finalize()
    assert code(lambda: sm.create_page_set([0, 1])) == 5
    sm.close()


def test_match_images_with_video_on_a_subset(tmp_path, capi, synth):
    """The upstream README's "lecture1 <-> video1, lecture2 <-> video2" in one process: one page analysis, each video matched
    against its own lecture's images through a page set, equal to a matcher of that lecture alone."""
    from PIL import Image
    from slideo_amd import matching as mt

    class Page:
        def __init__(self, path, nr): self.path, self.page_nr = path, nr
        def get_path(self): return self.path
        def __eq__(self, o): return isinstance(o, Page) and o.page_nr == self.page_nr
        def __hash__(self): return self.page_nr

    pages = synth.pages(8, 800, 450, seed=31)
    imgs = []
    for i, p in enumerate(pages):
        path = str(tmp_path / ("p%d.png" % i))
        Image.fromarray(p[:, :, ::-1]).save(path)
        imgs.append(Page(path, i))
    lecture2 = imgs[4:]
    frames, truth, _ = synth.frames(pages[4:], 6, 640, 360, seed=12)
    video = str(tmp_path / "v2.raw")
    mt.RawVideo.write(video, np.repeat(frames, 5, axis=0), fps=1.0)
    rep = mt.ProgressReporter(lambda *a: None)
    cfg = small_cfg(capi)
    vm = mt.HipImageVideoMatcher(cfg, device=0).create_video_matcher(imgs, rep)
    got = vm.match_images_with_video(video, rep, images=lecture2).process()
    alone = mt.HipImageVideoMatcher(cfg, device=0).create_video_matcher(lecture2, rep)
    want = alone.match_images_with_video(video, rep).process()
    assert [(x.video_frame_idx, x.image) for x in got] == [(x.video_frame_idx, x.image) for x in want]
    assert all(x.image is None or x.image in lecture2 for x in got)
    assert any(x.image is not None for x in got)
    # the set is released and set 0 selected again: the whole deck as before
    assert vm._m.page_set_info(0)["n_pages"] == 8
    with pytest.raises(ValueError):
        vm.match_images_with_video(video, rep, images=[Page("elsewhere", 99)])
