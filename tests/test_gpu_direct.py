"""The direct page look-up (include/slideo_amd.h "Direct page look-up") held to its definition.

The reference for every SSD is numpy in int64 over Matcher.small_image(frame) and Matcher.page_small(page); the similarity is the
numpy restatement of the host expression (tests/gate_mask_ref.py similarity); the reference for every frame that is not direct is
match_frames on exactly those frames, on a second matcher.  The look-up's own output is never the reference.

Shapes: the cfg0 shapes (640x360 frames, 800x450 pages: both have 461x259 small images, L = 358 197 bytes, odd) and a second config
with small_area 1200 (46x26 small images, L = 3 588: no multiple of the K granule).  The deck has five pages, the third of
them 4:3 (another small size).
"""
import os

import numpy as np
import pytest

import gate_mask_ref as gref
import yuv420_ref as yref
from conftest import small_cfg
from slideo_amd import _capi

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
UNCHANGED = (-1, 0.0, 0, 0)
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
W, H = 640, 360


def _matcher(capi, pages, cfg=None, t=None):
    m = capi.Matcher(cfg if cfg is not None else small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    if t is not None:
        m.set_direct_similarity(t)
    return m


def _np_ssd(smalls, page_smalls):
    """int64 [n, P]: the SSD of every small image with every page's; -1 where the sizes differ."""
    out = np.full((len(smalls), len(page_smalls)), -1, np.int64)
    for i, s in enumerate(smalls):
        for p, q in enumerate(page_smalls):
            if q.shape == s.shape:
                d = s.astype(np.int64) - q.astype(np.int64)
                out[i, p] = int((d * d).sum())
    return out


def _np_best(ssd, eligible=None):
    """Per row of _np_ssd: (best ssd, the lowest page with it) over the pages of the row's size (and of `eligible`); (-1, -1): none."""
    best = []
    for row in ssd:
        ok = [p for p in range(len(row)) if row[p] >= 0 and (eligible is None or p in eligible)]
        if not ok:
            best.append((-1, -1))
            continue
        v = min(int(row[p]) for p in ok)
        best.append((v, min(p for p in ok if int(row[p]) == v)))
    return best


def _sims(best, npx):
    return np.array([gref.similarity(b, npx) if b >= 0 else np.float32(-1) for b, _ in best], np.float32)


def _noisy(img, rng, amp=3):
    return np.clip(img.astype(np.int16) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def deck(capi, synth):
    """-> (pages: four 800x450 and, third, one 800x600; a finalized matcher over them; their small images)."""
    wide = synth.pages(4, 800, 450, threads=NCPU)
    tall = synth.pages(1, 800, 600, seed=77, threads=NCPU)
    pages = [wide[0], wide[1], tall[0], wide[2], wide[3]]
    r = _matcher(capi, pages)
    ps = [r.page_small(p) for p in range(5)]
    assert [q.shape for q in ps] == [(259, 461, 3)] * 2 + [(300, 400, 3)] + [(259, 461, 3)] * 2
    yield pages, r, ps
    r.close()


@pytest.fixture(scope="module")
def stream(capi, synth, deck):
    """A stream of holds mixing (a) pages resized to the frame size with noise and (b) the synthetic transformed frames.
    -> (seq [n, H, W, 3], kind [n]: 'a' / 'b', distinct: index of each frame's image)."""
    pages, r, _ = deck
    rng = np.random.default_rng(5)
    wide = [0, 1, 3, 4]
    full = [_noisy(r.reduce(pages[p], W, H), rng) for p in (0, 3, 1, 4, 0, 3)]
    moved, _, _ = synth.frames(np.stack([pages[p] for p in wide]), 6, W, H, threads=NCPU)
    images, kinds = [], []
    for j in range(6):
        images += [full[j], moved[j]]
        kinds += ["a", "b"]
    seq, kind, which = [], [], []
    for j, img in enumerate(images):
        for _ in range(int(rng.integers(1, 6))):
            seq.append(img); kind.append(kinds[j]); which.append(j)
    return np.stack(seq), np.array(kind), np.array(which), images


def _split(smalls, kind, ps, eligible=None):
    """numpy alone: best page and similarity per frame, and a t that puts every (a) frame at >= t and every (b) frame below it."""
    best = _np_best(_np_ssd(smalls, ps), eligible)
    sims = _sims(best, smalls[0].shape[0] * smalls[0].shape[1])
    lo, hi = float(sims[kind == "b"].max()), float(sims[kind == "a"].min())
    assert lo < hi, "the transformed frames are less similar to every page than the full-screen ones to theirs"
    t = float(np.float32((lo + hi) / 2))
    assert (sims[kind == "a"] >= np.float32(t)).all() and (sims[kind == "b"] < np.float32(t)).all()
    return best, sims, t


def _expect(r, seq, changed, best, sims, t, yuv=None):
    """The definition: verdicts of all frames and the traces of the frames that go through the pipeline (match_frames of exactly
    those on r), from the t = 0 flags and numpy's best pages."""
    direct = np.array([changed[i] and best[i][1] >= 0 and sims[i] >= np.float32(t) for i in range(len(seq))])
    rest = np.nonzero(changed & ~direct)[0]
    want = np.zeros(len(seq), _capi.VERDICT_DTYPE)
    want[:] = UNCHANGED
    traces = []
    if len(rest):
        want[rest] = r.match_frames(seq[rest]) if yuv is None else r.match_frames_yuv420(seq[rest], *yuv)
        traces = [r.last_candidates(k).tobytes() for k in range(len(rest))]
    for i in np.nonzero(direct)[0]:
        want[i] = (best[i][1], sims[i], 0, 0)
    return direct, want, traces


def _check(got, base, want, traces, m, what):
    changed, sims, v = got
    assert np.array_equal(changed, base[0]), (what, "flags")
    assert np.array_equal(sims.view(np.uint32), base[1].view(np.uint32)), (what, "similarities")
    assert v.tobytes() == want.tobytes(), (what, [(i, v[i], want[i]) for i in range(len(v)) if v[i] != want[i]][:4])
    for k, tr in enumerate(traces):
        assert m.last_candidates(k).tobytes() == tr, (what, "trace of pipeline frame %d" % k)


# ---- the tap against numpy, exact -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 33])
def test_tap_random_small_images(deck, n):
    """n = 3 at odd L: the three images sit at three byte alignments; 33: more than one 32-row tile."""
    _, r, ps = deck
    smalls = np.random.default_rng(n).integers(0, 256, (n, 259, 461, 3), dtype=np.uint8)
    want = _np_ssd(smalls, ps)
    got = r.page_small_ssd(smalls)
    assert got.shape == (n, 5) and (got[:, 2] == U64_MAX).all()
    wide = [0, 1, 3, 4]
    assert np.array_equal(got[:, wide].astype(np.int64), want[:, wide])


def test_tap_a_pages_own_small_image_and_the_other_class(deck):
    _, r, ps = deck
    got = r.page_small_ssd(np.stack([ps[3], ps[0], ps[4]]))
    assert got[0, 3] == 0 and got[1, 0] == 0 and got[2, 4] == 0
    assert np.array_equal(got[:, [0, 1, 3, 4]].astype(np.int64), _np_ssd([ps[3], ps[0], ps[4]], ps)[:, [0, 1, 3, 4]])
    tall = r.page_small_ssd(ps[2][None])
    assert tall[0, 2] == 0 and (tall[0, [0, 1, 3, 4]] == U64_MAX).all()


def test_tap_extremes_need_the_accumulators_drained(capi, synth, deck):
    """All-0 and all-255 small images at 461x259: <a', b'> is +-5.9e9, far outside one i32 accumulator."""
    pages, _, _ = deck
    black, white = np.zeros((450, 800, 3), np.uint8), np.full((450, 800, 3), 255, np.uint8)
    m = _matcher(capi, [black, white, pages[0]])
    ps = [m.page_small(p) for p in range(3)]
    assert not ps[0].any() and (ps[1] == 255).all()
    smalls = np.stack([np.zeros((259, 461, 3), np.uint8), np.full((259, 461, 3), 255, np.uint8)])
    got = m.page_small_ssd(smalls)
    top = 255 * 255 * 3 * 461 * 259
    assert got[0, 0] == 0 and got[0, 1] == top and got[1, 0] == top and got[1, 1] == 0
    assert np.array_equal(got.astype(np.int64), _np_ssd(smalls, ps))
    m.close()


@pytest.mark.parametrize("n", [1, 3, 33])
def test_tap_ragged_k(capi, deck, n):
    """small_area 1200: 46x26 small images, 3 588 bytes — the K padding and the last, short K chunk."""
    pages, _, _ = deck
    m = _matcher(capi, pages, small_cfg(capi, small_area=1200))
    ps = [m.page_small(p) for p in range(5)]
    sh, sw = ps[0].shape[:2]
    assert (sw * sh * 3) % 64 != 0 and ps[2].shape != ps[0].shape
    smalls = np.random.default_rng(100 + n).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    smalls[0] = ps[1]
    got = m.page_small_ssd(smalls)
    want = _np_ssd(smalls, ps)
    assert got[0, 1] == 0 and (got[:, 2] == U64_MAX).all()
    assert np.array_equal(got[:, [0, 1, 3, 4]].astype(np.int64), want[:, [0, 1, 3, 4]])
    m.close()


# ---- the gated calls ----------------------------------------------------------------------------------------------------------------

def test_t_zero_changes_nothing(capi, deck, stream):
    pages, _, _ = deck
    seq = stream[0]
    a, b = _matcher(capi, pages), _matcher(capi, pages, t=0.0)
    assert b.direct_similarity == 0.0
    ga, gb = a.match_changed_frames(seq), b.match_changed_frames(seq)
    for x, y in zip(ga, gb):
        assert x.tobytes() == y.tobytes()
    assert ga[0].any() and not ga[0].all()
    for k in range(int(ga[0].sum())):
        assert a.last_candidates(k).tobytes() == b.last_candidates(k).tobytes()
    assert np.array_equal(a.gate_last_small(), b.gate_last_small())
    a.close(); b.close()


@pytest.fixture(scope="module")
def definition(capi, deck, stream):
    """numpy's split of the stream, the t = 0 run and what the definition gives for every frame (computed once)."""
    pages, r, ps = deck
    seq, kind, which, images = stream
    img_smalls = [r.small_image(im) for im in images]
    best, sims, t = _split([img_smalls[j] for j in which], kind, ps)
    base_m = _matcher(capi, pages)
    base = base_m.match_changed_frames(seq)
    last = base_m.gate_last_small()
    base_m.close()
    direct, want, traces = _expect(r, seq, base[0], best, sims, t)
    assert direct.any() and (base[0] & ~direct).any() and not base[0].all()
    return t, base, last, want, traces


def test_definition_host_bgr(capi, deck, stream, definition):
    pages, seq = deck[0], stream[0]
    t, base, last, want, traces = definition
    m = _matcher(capi, pages, t=t)
    assert m.direct_similarity == np.float32(t)
    _check(m.match_changed_frames(seq), base, want, traces, m, "host bgr")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


def test_definition_submit_collect(capi, deck, stream, definition):
    """Device frames, units of different sizes in flight."""
    import torch
    pages, seq = deck[0], stream[0]
    t, base, last, want, traces = definition
    n = len(seq)
    m = _matcher(capi, pages, t=t)
    d = torch.from_numpy(seq).cuda()
    fb = W * H * 3
    sizes, got, pend, i = [1, 7, 5, 3, 11], [], [], 0
    while i < n:
        c = min(sizes[len(got) + len(pend)] if len(got) + len(pend) < len(sizes) else 6, n - i)
        if len(pend) == m.max_in_flight():
            got.append(m.collect_changed(pend.pop(0)))
        pend.append(m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H))
        i += c
    got += [m.collect_changed(tk) for tk in pend]
    _check(tuple(np.concatenate([g[j] for g in got]) for j in range(3)), base, want, traces, m, "stream")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


def test_definition_group_of_two(capi, deck, stream, definition):
    pages, seq = deck[0], stream[0]
    t, base, last, want, traces = definition
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    g.set_direct_similarity(t)
    assert g.direct_similarity == np.float32(t)
    _check(g.match_changed_frames(seq), base, want, traces, g, "group of two")
    assert np.array_equal(g.gate_last_small(), last)
    g.close()


def test_definition_nv12(capi, deck, stream):
    pages, r, ps = deck
    seq, kind, which, images = stream
    L, fb = capi.yuv420_layout("nv12", W, H)
    img_yuv = yref.frames_to_yuv(np.stack(images), L, fb)
    yuv = img_yuv[which]
    img_smalls = [r.small_image(r.yuv420_to_bgr(f, W, H, L)) for f in img_yuv]
    best, sims, t = _split([img_smalls[j] for j in which], kind, ps)
    base_m = _matcher(capi, pages)
    base = base_m.match_changed_frames_yuv420(yuv, W, H, L)
    last = base_m.gate_last_small()
    base_m.close()
    direct, want, traces = _expect(r, yuv, base[0], best, sims, t, yuv=(W, H, L))
    assert direct.any() and (base[0] & ~direct).any()
    m = _matcher(capi, pages, t=t)
    _check(m.match_changed_frames_yuv420(yuv, W, H, L), base, want, traces, m, "host nv12")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


def test_ties_go_to_the_lower_page(capi, deck):
    pages, r, _ = deck
    twice = [pages[0], pages[1], pages[1], pages[3]]
    m = _matcher(capi, twice, t=0.9)
    frame = _noisy(r.reduce(pages[1], W, H), np.random.default_rng(9))
    ps = [m.page_small(p) for p in range(4)]
    assert np.array_equal(ps[1], ps[2])
    best = _np_best(_np_ssd([m.small_image(frame)], ps))
    sims = _sims(best, 461 * 259)
    assert best[0][1] == 1 and sims[0] >= np.float32(0.9)
    ch, _, v = m.match_changed_frames(frame[None])
    assert ch[0] and tuple(v[0]) == (1, sims[0], 0, 0)
    got = m.page_small_ssd(m.small_image(frame)[None])
    assert got[0, 1] == got[0, 2] == best[0][0]
    m.close()


def test_page_set_excluding_the_true_page(capi, deck):
    pages, r, ps = deck
    rng = np.random.default_rng(13)
    frames = np.stack([_noisy(r.reduce(pages[1], W, H), rng), _noisy(r.reduce(pages[4], W, H), rng)])
    smalls = [r.small_image(f) for f in frames]
    in_set = [0, 3, 4]
    best = _np_best(_np_ssd(smalls, ps), set(in_set))
    sims = _sims(best, 461 * 259)
    full = _sims(_np_best(_np_ssd(smalls, ps)), 461 * 259)
    t = float(np.float32((float(sims[0]) + float(min(full[0], sims[1]))) / 2))
    assert sims[0] < np.float32(t) <= sims[1] and full[0] >= np.float32(t) and best[1][1] == 4 and best[0][1] != 1
    m = _matcher(capi, pages, t=t)
    sid, rid = m.create_page_set(in_set), r.create_page_set(in_set)
    m.use_page_set(sid); r.use_page_set(rid)
    try:
        ch, _, v = m.match_changed_frames(frames)
        assert ch.all()
        assert tuple(v[1]) == (4, sims[1], 0, 0)
        ref = r.match_frames(frames[:1])
        assert v[:1].tobytes() == ref.tobytes() and v[0]["page_idx"] != 1
        assert m.last_candidates(0).tobytes() == r.last_candidates(0).tobytes()
        # the whole deck again: the frame of page 1 is direct for it
        m.use_page_set(0); m.gate_reset(None)
        ch, _, v = m.match_changed_frames(frames[:1])
        assert tuple(v[0]) == (1, full[0], 0, 0)
    finally:
        r.use_page_set(0); r.release_page_set(rid)
    m.close()


def test_size_classes(capi, deck):
    """A 4:3 frame: direct for the deck's 4:3 page; never direct over a deck without a page of its small size."""
    pages, r, ps = deck
    frame = _noisy(r.reduce(pages[2], 640, 480), np.random.default_rng(17))
    small = r.small_image(frame)
    assert small.shape == ps[2].shape
    best = _np_best(_np_ssd([small], ps))
    sims = _sims(best, small.shape[0] * small.shape[1])
    assert best[0][1] == 2 and sims[0] >= np.float32(0.9)
    m = _matcher(capi, pages, t=0.9)
    ch, _, v = m.match_changed_frames(frame[None])
    assert ch[0] and tuple(v[0]) == (2, sims[0], 0, 0)
    m.close()
    wide = [pages[p] for p in (0, 1, 3, 4)]
    a, b = _matcher(capi, wide), _matcher(capi, wide, t=1e-6)
    ga, gb = a.match_changed_frames(frame[None]), b.match_changed_frames(frame[None])
    assert ga[0][0] and ga[2].tobytes() == gb[2].tobytes() and not (gb[2][0]["page_idx"] >= 0 and gb[2][0]["inliers"] == 0)
    assert a.last_candidates(0).tobytes() == b.last_candidates(0).tobytes()
    a.close(); b.close()


def test_refusals_and_arguments(capi, deck, stream):
    import torch
    pages, r, _ = deck
    seq = stream[0]
    m = _matcher(capi, pages)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(capi.SlideoError) as e:
            m.set_direct_similarity(bad)
        assert e.value.code == 1 and m.direct_similarity == 0.0
    mask = np.full((H, W), 255, np.uint8)
    mask[:40] = 0
    # the mask under the GATE scope first, then t > 0
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(mask)
    with pytest.raises(capi.SlideoError) as e:
        m.set_direct_similarity(0.9)
    assert e.value.code == 5 and m.direct_similarity == 0.0
    # t > 0 first, then each of the two calls that would complete the combination
    m.set_frame_mask(None)
    m.set_direct_similarity(0.9)
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask(mask)
    assert e.value.code == 5 and m.frame_mask_info is None
    m.set_frame_mask_scope(capi.MASK_DETECT)
    m.set_frame_mask(mask)                                         # DETECT alone is fine
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    assert e.value.code == 5 and m.frame_mask_scope == capi.MASK_DETECT and m.direct_similarity == np.float32(0.9)
    m.set_frame_mask(None)
    # a busy matcher
    d = torch.from_numpy(seq[:2]).cuda()
    tk = m.submit_changed_dev(d.data_ptr(), 2, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_direct_similarity(0.5)
    assert e.value.code == 4
    m.collect_changed(tk)
    # the plain calls do not look up
    plain = m.match_frames(seq[:6])
    assert plain.tobytes() == r.match_frames(seq[:6]).tobytes()
    assert (plain["page_idx"] < 0).all() or (plain["inliers"][plain["page_idx"] >= 0] > 0).all()
    m.close()


def test_definition_under_a_working_size(capi, deck, stream, definition):
    """Every pixel of the stream's first frames doubled to 1280x720: under a working size of 640x360 the reduced frame is the
    640x360 frame itself (INTER_AREA over 2x2 equal pixels), so the call returns what the definition gives for those frames."""
    pages, seq = deck[0], stream[0]
    t, base, _, want, traces = definition
    k = 14
    big = np.ascontiguousarray(seq[:k].repeat(2, axis=1).repeat(2, axis=2))
    assert big.shape == (k, 2 * H, 2 * W, 3)
    is_direct = (want["page_idx"][:k] >= 0) & (want["inliers"][:k] == 0)
    piped = int((base[0][:k] & ~is_direct).sum())
    assert is_direct.any() and piped > 0
    m = _matcher(capi, pages, t=t)
    m.set_working_size(W, H)
    assert np.array_equal(m.reduce(big[0], W, H), seq[0])
    _check(m.match_changed_frames(big), (base[0][:k], base[1][:k]), want[:k], traces[:piped], m, "working size")
    assert np.array_equal(m.gate_last_small(), m.small_image(seq[k - 1]))
    m.close()


def test_group_setter_validates_before_any_member_changes(capi, deck, stream):
    """A bad t, a member under MASK_GATE and a busy member each refuse the group's call and leave EVERY member's t as it was;
    the group's own mask calls refuse the combination in both orders."""
    import torch
    pages, seq = deck[0], stream[0]
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(pages)); g.finalize()
    members = [g.member(0), g.member(1)]

    def ts():
        return [mm.direct_similarity for mm in members]
    g.set_direct_similarity(0.75)
    assert ts() == [0.75, 0.75]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(capi.SlideoError) as e:
            g.set_direct_similarity(bad)
        assert e.value.code == 1 and ts() == [0.75, 0.75]
    # the LAST member alone under a mask with the GATE scope (t = 0 meanwhile, or the member's own calls would refuse)
    mask = np.full((H, W), 255, np.uint8)
    mask[:40] = 0
    g.set_direct_similarity(0.0)
    members[1].set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    members[1].set_frame_mask(mask)
    with pytest.raises(capi.SlideoError) as e:
        g.set_direct_similarity(0.9)
    assert e.value.code == 5 and ts() == [0.0, 0.0]
    members[1].set_frame_mask(None)
    members[1].set_frame_mask_scope(capi.MASK_DETECT)
    # the last member alone busy
    g.set_direct_similarity(0.75)
    d = torch.from_numpy(seq[:2]).cuda()
    tk = members[1].submit_changed_dev(d.data_ptr(), 2, W, H)
    with pytest.raises(capi.SlideoError) as e:
        g.set_direct_similarity(0.5)
    assert e.value.code == 4 and ts() == [0.75, 0.75]
    members[1].collect_changed(tk)
    members[1].gate_reset(None)
    # the group's mask calls: the mask under the GATE scope first, then t > 0 ...
    g.set_direct_similarity(0.0)
    g.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    g.set_frame_mask(mask)
    with pytest.raises(capi.SlideoError) as e:
        g.set_direct_similarity(0.9)
    assert e.value.code == 5 and ts() == [0.0, 0.0]
    # ... and t > 0 first, then each of the two calls that would complete the combination
    g.set_frame_mask(None)
    g.set_direct_similarity(0.9)
    with pytest.raises(capi.SlideoError) as e:
        g.set_frame_mask(mask)
    assert e.value.code == 5 and all(mm.frame_mask_info is None for mm in members)
    g.set_frame_mask_scope(capi.MASK_DETECT)
    g.set_frame_mask(mask)                                         # DETECT alone is fine
    with pytest.raises(capi.SlideoError) as e:
        g.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    assert e.value.code == 5 and [mm.frame_mask_scope for mm in members] == [capi.MASK_DETECT] * 2 and ts() == [np.float32(0.9)] * 2
    g.close()
