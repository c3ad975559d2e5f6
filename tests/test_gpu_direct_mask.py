"""The direct look-up scope SLIDEO_DIRECT_VALID (include/slideo_amd.h "Direct look-up scope") held to its definition: the direct page
look-up over the valid pixels of the gate's validity map.

References are numpy only: gate_mask_ref.validity_map (over the CPU to_small_image) for the map, gate_mask_ref.masked_ssd in int64
over Matcher.small_image(frame) and Matcher.page_small(page), gate_mask_ref.similarity, and match_frames on a second matcher (under
the same mask) for the frames that are not direct.  The look-up's own output is never the reference.

Shapes: those of test_gpu_direct.py (640x360 frames and 800x450 pages: 461x259 small images, L = 358 197 bytes, odd, so the images
of a unit start at every byte alignment) and a second config with small_area 1200 (small images of about 46x26 pixels whose byte
count is no multiple of the K granule of 128).
The deck has five pages, the third of them 4:3 (another small size).  A pixel is three bytes, so the weights change inside dwords
under every mask here.
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
HOLE = (170, 350, 380, 630)            # rows, columns of the hole in the 640x360 mask: 45 000 of 230 400 pixels, about 20 %
INSET = (171, 349, 381, 629)           # the inset: one pixel inside the hole on every side
WIDE = [0, 1, 3, 4]
AREAS = {"A": 120000, "B": 1200}       # small_area of the two configs (A: slideo_config_default's)


def _cfg(capi, key):
    return small_cfg(capi) if key == "A" else small_cfg(capi, small_area=AREAS["B"])


def _one_pixel_mask(sw, sh):
    """Nonzero over exactly the source pixels that small pixel (sh // 2, sw // 3) averages: its neighbours reach outside."""
    iy, ix = sh // 2, sw // 3
    sx, sy = W / sw, H / sh
    m = np.zeros((H, W), np.uint8)
    m[int(np.floor(iy * sy)):int(np.ceil((iy + 1) * sy)), int(np.floor(ix * sx)):int(np.ceil((ix + 1) * sx))] = 255
    return m


def _masks(sw, sh):
    hole = np.full((H, W), 255, np.uint8)
    hole[HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = 0
    tail_invalid = np.full((H, W), 255, np.uint8)
    tail_invalid[H - 20:, W - 30:] = 0
    tail_valid = np.full((H, W), 255, np.uint8)
    tail_valid[:40, :60] = 0
    return {"hole": hole, "tail_invalid": tail_invalid, "tail_valid": tail_valid, "one": _one_pixel_mask(sw, sh),
            "all": np.full((H, W), 255, np.uint8)}


def _noisy(img, rng, amp=3):
    return np.clip(img.astype(np.int16) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def _with_inset(frames, seed):
    """A random texture in the inset, renewed on every frame."""
    rng = np.random.default_rng(seed)
    out = np.array(frames, copy=True)
    y0, y1, x0, x1 = INSET
    for f in out:
        f[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    return out


def _matcher(capi, pages, cfg=None, mask=None, mask_scope=None, scope=None, t=None):
    """The mirrors' order: mask scope, mask, direct scope, direct similarity."""
    m = capi.Matcher(cfg if cfg is not None else small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    if mask_scope is not None:
        m.set_frame_mask_scope(mask_scope)
    if mask is not None:
        m.set_frame_mask(mask)
    if scope is not None:
        m.set_direct_scope(scope)
    if t is not None:
        m.set_direct_similarity(t)
    return m


def _np_ssd(smalls, page_smalls, valid=None):
    """int64 [n, P]: the SSD over the valid pixels (None: all) of every small image with every page's; -1 where the sizes differ."""
    out = np.full((len(smalls), len(page_smalls)), -1, np.int64)
    for i, s in enumerate(smalls):
        for p, q in enumerate(page_smalls):
            if q.shape == s.shape:
                out[i, p] = gref.masked_ssd(s, q, np.ones(s.shape[:2], bool) if valid is None else valid)
    return out


def _np_best(ssd, eligible=None):
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


@pytest.fixture(scope="module")
def deck(capi, synth):
    """-> the pages: four 800x450 and, third, one 800x600."""
    wide = synth.pages(4, 800, 450, threads=NCPU)
    tall = synth.pages(1, 800, 600, seed=77, threads=NCPU)
    return [wide[0], wide[1], tall[0], wide[2], wide[3]]


@pytest.fixture(scope="module")
def taps(capi, oracle, deck):
    """Per config: a finalized matcher under DETECT | GATE, its pages' small images, 70 random small images and the masks with their
    numpy validity maps (each with n_valid > 0)."""
    out = {}
    for key in AREAS:
        m = _matcher(capi, deck, _cfg(capi, key), mask_scope=capi.MASK_DETECT | capi.MASK_GATE)
        ps = [m.page_small(p) for p in range(5)]
        sh, sw = ps[0].shape[:2]
        assert ((sw, sh) == (461, 259) if key == "A" else sw * sh <= 1200) and (sw * sh * 3) % 128 != 0 and ps[2].shape != ps[0].shape
        smalls = np.random.default_rng(sw).integers(0, 256, (70, sh, sw, 3), dtype=np.uint8)
        smalls[1] = ps[3]
        masks = {}
        for name, mask in _masks(sw, sh).items():
            valid, nv = gref.validity_map(oracle, mask, AREAS[key])
            assert valid.shape == (sh, sw) and nv > 0, (key, name)
            masks[name] = (mask, valid, nv)
        assert not masks["tail_invalid"][1][-1, -1] and masks["tail_valid"][1][-1, -1]        # the ragged tail, both ways
        assert masks["one"][2] == 1 and masks["all"][2] == sw * sh and 0.7 < masks["hole"][2] / (sw * sh) < 0.85
        out[key] = dict(m=m, ps=ps, smalls=smalls, masks=masks)
    yield out
    for v in out.values():
        v["m"].close()


# ---- 1. the tap against numpy, exact ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hole", "tail_invalid", "tail_valid", "one", "all"])
@pytest.mark.parametrize("key", ["A", "B"])
def test_tap_against_numpy(capi, taps, key, name):
    """n = 1, 3, 33, 70: images at every byte alignment (L odd in A), one and two frame tiles, pad rows.  The mask is replaced from
    case to case on one matcher, so the masked page norms follow the map here too."""
    d = taps[key]
    m, ps, smalls = d["m"], d["ps"], d["smalls"]
    mask, valid, nv = d["masks"][name]
    m.set_frame_mask(mask)
    got_map, got_nv = m.frame_mask_small()
    assert got_nv == nv and np.array_equal(got_map, valid)
    want = _np_ssd(smalls, ps, valid)
    for n in (1, 3, 33, 70):
        got = m.page_small_ssd_valid(smalls[:n])
        assert got.shape == (n, 5) and (got[:, 2] == U64_MAX).all(), (key, name, n)
        assert np.array_equal(got[:, WIDE].astype(np.int64), want[:n, WIDE]), (key, name, n)
    assert want[1, 3] == 0
    if name == "all":                                               # every pixel valid: the unmasked tap's SSDs
        assert np.array_equal(m.page_small_ssd_valid(smalls[:3]), m.page_small_ssd(smalls[:3]))
    else:                                                           # the unmasked tap is not disturbed by the masked norms
        assert np.array_equal(m.page_small_ssd(smalls[:3])[:, WIDE].astype(np.int64), _np_ssd(smalls[:3], ps)[:, WIDE])


def test_tap_extremes_need_the_accumulators_drained(capi, deck, taps):
    """An all-0 image against an all-255 page under the hole mask at 461x259: <a'_m, b'> is far outside one i32 accumulator."""
    mask, valid, nv = taps["A"]["masks"]["hole"]
    black, white = np.zeros((450, 800, 3), np.uint8), np.full((450, 800, 3), 255, np.uint8)
    m = _matcher(capi, [black, white, deck[0]], mask=mask, mask_scope=capi.MASK_DETECT | capi.MASK_GATE)
    ps = [m.page_small(p) for p in range(3)]
    assert not ps[0].any() and (ps[1] == 255).all()
    smalls = np.stack([np.zeros((259, 461, 3), np.uint8), np.full((259, 461, 3), 255, np.uint8)])
    got = m.page_small_ssd_valid(smalls)
    top = 255 * 255 * 3 * nv
    assert got[0, 0] == 0 and got[0, 1] == top and got[1, 0] == top and got[1, 1] == 0
    assert np.array_equal(got.astype(np.int64), _np_ssd(smalls, ps, valid))
    m.close()


def test_tap_states_and_arguments(capi, deck, taps):
    mask = taps["A"]["masks"]["hole"][0]
    smalls = taps["A"]["smalls"][:1]
    m = _matcher(capi, deck)
    for prep in (lambda: None, lambda: m.set_frame_mask(mask)):     # no mask; a mask under DETECT alone: no map in force
        prep()
        with pytest.raises(capi.SlideoError) as e:
            m.page_small_ssd_valid(smalls)
        assert e.value.code == 4
    m.set_frame_mask_scope(capi.MASK_GATE)
    assert m.page_small_ssd_valid(smalls).shape == (1, 5)           # whatever t and the direct scope are
    for other in (np.zeros((1, 300, 400, 3), np.uint8), np.zeros((1, 26, 46, 3), np.uint8)):
        with pytest.raises(capi.SlideoError) as e:
            m.page_small_ssd_valid(other)
        assert e.value.code == 1
    m.set_frame_mask(None)
    with pytest.raises(capi.SlideoError) as e:
        m.page_small_ssd_valid(smalls)
    assert e.value.code == 4
    m.close()


# ---- 2. the definition ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref(capi, deck, taps):
    """The second matcher: under the hole mask and DETECT | GATE, t = 0 — small images, match_frames, traces."""
    r = _matcher(capi, deck, mask=taps["A"]["masks"]["hole"][0], mask_scope=capi.MASK_DETECT | capi.MASK_GATE)
    yield r
    r.close()


@pytest.fixture(scope="module")
def stream(capi, synth, deck, ref):
    """Holds of (a) pages resized to the frame size with noise and (b) the synthetic transformed frames, alternating; on top of every
    frame an inset of its own where the mask has its hole.  -> (seq [n, H, W, 3], kind [n])."""
    rng = np.random.default_rng(5)
    full = [_noisy(ref.reduce(deck[p], W, H), rng) for p in (0, 3, 1, 4)]
    moved, _, _ = synth.frames(np.stack([deck[p] for p in WIDE]), 4, W, H, threads=NCPU)
    seq, kind = [], []
    for j in range(4):
        for img, k in ((full[j], "a"), (moved[j], "b")):
            for _ in range(int(rng.integers(1, 4))):
                seq.append(img); kind.append(k)
    return _with_inset(np.stack(seq), 11), np.array(kind)


def _split(smalls, kind, ps, valid, nv, eligible=None):
    """numpy alone: best page and masked similarity per frame, a t that puts every (a) frame at >= t and every (b) frame below it
    — and below which at least one (a) frame's WHOLE-image similarity lies: the mask matters."""
    best = _np_best(_np_ssd(smalls, ps, valid), eligible)
    sims = _sims(best, nv)
    lo, hi = float(sims[kind == "b"].max()), float(sims[kind == "a"].min())
    assert lo < hi, "the transformed frames are less similar to every page than the full-screen ones to theirs"
    t = float(np.float32((lo + hi) / 2))
    assert (sims[kind == "a"] >= np.float32(t)).all() and (sims[kind == "b"] < np.float32(t)).all()
    whole = _sims(_np_best(_np_ssd(smalls, ps), eligible), smalls[0].shape[0] * smalls[0].shape[1])
    assert (whole[kind == "a"] < np.float32(t)).any(), "the inset pushes a full-screen frame's whole-image similarity below t"
    return best, sims, t


def _expect(r, seq, changed, best, sims, t, yuv=None):
    """The definition: verdicts of all frames and the traces of the frames that go through the pipeline (match_frames of exactly
    those on r, under the same mask), from the t = 0 flags and numpy's best pages."""
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


def _valid_matcher(capi, pages, mask, t):
    return _matcher(capi, pages, mask=mask, mask_scope=capi.MASK_DETECT | capi.MASK_GATE, scope=capi.DIRECT_VALID, t=t)


@pytest.fixture(scope="module")
def definition(capi, deck, taps, ref, stream):
    """numpy's split of the stream under the hole mask, the t = 0 run under the same mask and what the definition gives."""
    seq, kind = stream
    mask, valid, nv = taps["A"]["masks"]["hole"]
    ps = taps["A"]["ps"]
    smalls = [ref.small_image(f) for f in seq]
    best, sims, t = _split(smalls, kind, ps, valid, nv)
    ref.gate_reset(None)
    base = ref.match_changed_frames(seq)
    last = ref.gate_last_small()
    direct, want, traces = _expect(ref, seq, base[0], best, sims, t)
    # under the mask the holds are unchanged although every frame has an inset of its own
    assert direct.any() and (base[0] & ~direct).any() and not base[0].all()
    return t, base, last, want, traces


def test_definition_host_bgr(capi, deck, taps, stream, definition):
    t, base, last, want, traces = definition
    m = _valid_matcher(capi, deck, taps["A"]["masks"]["hole"][0], t)
    assert m.direct_scope == capi.DIRECT_VALID and m.direct_similarity == np.float32(t)
    _check(m.match_changed_frames(stream[0]), base, want, traces, m, "host bgr")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


def test_definition_submit_collect(capi, deck, taps, stream, definition):
    """Device frames, units of different sizes in flight."""
    import torch
    seq = stream[0]
    t, base, last, want, traces = definition
    n = len(seq)
    m = _valid_matcher(capi, deck, taps["A"]["masks"]["hole"][0], t)
    d = torch.from_numpy(seq).cuda()
    fb = W * H * 3
    sizes, got, pend, i = [1, 4, 3, 2], [], [], 0
    while i < n:
        c = min(sizes[len(got) + len(pend)] if len(got) + len(pend) < len(sizes) else 5, n - i)
        if len(pend) == m.max_in_flight():
            got.append(m.collect_changed(pend.pop(0)))
        pend.append(m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H))
        i += c
    got += [m.collect_changed(tk) for tk in pend]
    _check(tuple(np.concatenate([g[j] for g in got]) for j in range(3)), base, want, traces, m, "stream")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


def test_definition_nv12(capi, deck, taps, ref, stream):
    seq, kind = stream
    mask, valid, nv = taps["A"]["masks"]["hole"]
    L, fb = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(seq, L, fb)
    smalls = [ref.small_image(ref.yuv420_to_bgr(f, W, H, L)) for f in yuv]
    best, sims, t = _split(smalls, kind, taps["A"]["ps"], valid, nv)
    ref.gate_reset(None)
    base = ref.match_changed_frames_yuv420(yuv, W, H, L)
    last = ref.gate_last_small()
    direct, want, traces = _expect(ref, yuv, base[0], best, sims, t, yuv=(W, H, L))
    assert direct.any() and (base[0] & ~direct).any()
    m = _valid_matcher(capi, deck, mask, t)
    _check(m.match_changed_frames_yuv420(yuv, W, H, L), base, want, traces, m, "host nv12")
    assert np.array_equal(m.gate_last_small(), last)
    m.close()


# ---- 3. the masked norms follow the map -------------------------------------------------------------------------------------------

def test_masked_norms_follow_the_map(capi, deck, taps, ref):
    """The mask is replaced between two gated calls on one matcher: the second call is numpy's under the second map."""
    ps, masks = taps["A"]["ps"], taps["A"]["masks"]
    frame = _with_inset(_noisy(ref.reduce(deck[3], W, H), np.random.default_rng(3))[None], 4)[0]
    small = ref.small_image(frame)
    m = _valid_matcher(capi, deck, masks["hole"][0], 0.5)
    for name in ("hole", "tail_invalid", "hole"):
        mask, valid, nv = masks[name]
        m.set_frame_mask(mask)
        m.gate_reset(None)
        best = _np_best(_np_ssd([small], ps, valid))
        sims = _sims(best, nv)
        assert best[0][1] == 3 and sims[0] >= np.float32(0.5)
        ch, _, v = m.match_changed_frames(frame[None])
        assert ch[0] and tuple(v[0]) == (3, sims[0], 0, 0), (name, v[0], best, sims)
        assert np.array_equal(m.page_small_ssd_valid(small[None])[:, WIDE].astype(np.int64), _np_ssd([small], ps, valid)[:, WIDE])
    # under the second map the inset is compared: another SSD than under the first
    assert _np_ssd([small], ps, masks["hole"][1])[0, 3] != _np_ssd([small], ps, masks["tail_invalid"][1])[0, 3]
    m.close()


# ---- 4. ties go to the lower page -------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lower_page(capi, deck, taps, ref):
    """Two pages differ only under the hole: their masked SSDs are equal, the lower page wins (the whole image names the higher)."""
    mask, valid, nv = taps["A"]["masks"]["hole"]
    other = deck[1].copy()
    y0, y1, x0, x1 = [int(v * 1.25) for v in HOLE]
    other[y0 + 8:y1 - 8, x0 + 8:x1 - 8] ^= 0xFF
    pages = [deck[0], other, deck[1], deck[3]]
    m = _valid_matcher(capi, pages, mask, 0.9)
    frame = _noisy(ref.reduce(deck[1], W, H), np.random.default_rng(9))
    ps = [m.page_small(p) for p in range(4)]
    small = m.small_image(frame)
    assert not np.array_equal(ps[1], ps[2]) and np.array_equal(ps[1][valid], ps[2][valid])
    masked, whole = _np_ssd([small], ps, valid), _np_ssd([small], ps)
    best = _np_best(masked)
    sims = _sims(best, nv)
    assert masked[0, 1] == masked[0, 2] and best[0][1] == 1 and sims[0] >= np.float32(0.9) and _np_best(whole)[0][1] == 2
    ch, _, v = m.match_changed_frames(frame[None])
    assert ch[0] and tuple(v[0]) == (1, sims[0], 0, 0)
    got = m.page_small_ssd_valid(small[None])
    assert got[0, 1] == got[0, 2] == best[0][0]
    m.close()


# ---- 5. page set and working size -------------------------------------------------------------------------------------------------

def test_page_set_excluding_the_true_page(capi, deck, taps, ref):
    mask, valid, nv = taps["A"]["masks"]["hole"]
    ps = taps["A"]["ps"]
    rng = np.random.default_rng(13)
    frames = _with_inset(np.stack([_noisy(ref.reduce(deck[1], W, H), rng), _noisy(ref.reduce(deck[4], W, H), rng)]), 14)
    smalls = [ref.small_image(f) for f in frames]
    in_set = [0, 3, 4]
    ssd = _np_ssd(smalls, ps, valid)
    best = _np_best(ssd, set(in_set))
    sims = _sims(best, nv)
    full = _sims(_np_best(ssd), nv)
    t = float(np.float32((float(sims[0]) + float(min(full[0], sims[1]))) / 2))
    assert sims[0] < np.float32(t) <= sims[1] and full[0] >= np.float32(t) and best[1][1] == 4 and best[0][1] != 1
    m = _valid_matcher(capi, deck, mask, t)
    sid, rid = m.create_page_set(in_set), ref.create_page_set(in_set)
    m.use_page_set(sid); ref.use_page_set(rid)
    try:
        ch, _, v = m.match_changed_frames(frames)
        assert ch.all()
        assert tuple(v[1]) == (4, sims[1], 0, 0)
        want = ref.match_frames(frames[:1])
        assert v[:1].tobytes() == want.tobytes() and v[0]["page_idx"] != 1
        assert m.last_candidates(0).tobytes() == ref.last_candidates(0).tobytes()
        # the whole deck again: the frame of page 1 is direct for it
        m.use_page_set(0); m.gate_reset(None)
        ch, _, v = m.match_changed_frames(frames[:1])
        assert tuple(v[0]) == (1, full[0], 0, 0)
    finally:
        ref.use_page_set(0); ref.release_page_set(rid)
    m.close()


def test_definition_under_a_working_size(capi, deck, taps, stream, definition):
    """Every pixel of the stream's first frames doubled to 1280x720: under a working size of 640x360 the reduced frame is the
    640x360 frame itself, and the mask is of the reduced size."""
    seq = stream[0]
    t, base, _, want, traces = definition
    k = 8
    big = np.ascontiguousarray(seq[:k].repeat(2, axis=1).repeat(2, axis=2))
    is_direct = (want["page_idx"][:k] >= 0) & (want["inliers"][:k] == 0)
    piped = int((base[0][:k] & ~is_direct).sum())
    assert is_direct.any() and piped > 0
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(deck)); m.finalize()
    m.set_working_size(W, H)
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(taps["A"]["masks"]["hole"][0])
    m.set_direct_scope(capi.DIRECT_VALID)
    m.set_direct_similarity(t)
    assert np.array_equal(m.reduce(big[0], W, H), seq[0])
    _check(m.match_changed_frames(big), (base[0][:k], base[1][:k]), want[:k], traces[:piped], m, "working size")
    assert np.array_equal(m.gate_last_small(), m.small_image(seq[k - 1]))
    m.close()


# ---- 6. the group -----------------------------------------------------------------------------------------------------------------

def test_group_of_two_equals_the_single_matcher(capi, deck, taps, stream, definition):
    t, base, last, want, traces = definition
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(deck)); g.finalize()
    g.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    g.set_frame_mask(taps["A"]["masks"]["hole"][0])
    g.set_direct_scope(capi.DIRECT_VALID)
    g.set_direct_similarity(t)
    assert g.direct_scope == capi.DIRECT_VALID and g.direct_similarity == np.float32(t)
    _check(g.match_changed_frames(stream[0]), base, want, traces, g, "group of two")
    assert np.array_equal(g.gate_last_small(), last)
    g.close()


def test_group_setter_validates_before_any_member_changes(capi, deck, taps, stream):
    import torch
    mask = taps["A"]["masks"]["hole"][0]
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(deck)); g.finalize()
    members = [g.member(0), g.member(1)]

    def scopes():
        return [mm.direct_scope for mm in members]
    assert scopes() == [capi.DIRECT_WHOLE] * 2
    g.set_direct_scope(capi.DIRECT_VALID)
    assert scopes() == [capi.DIRECT_VALID] * 2
    for bad in (2, 7, 0xFFFFFFFF):
        with pytest.raises(capi.SlideoError) as e:
            g.set_direct_scope(bad)
        assert e.value.code == 1 and scopes() == [capi.DIRECT_VALID] * 2
    # the LAST member alone holds the combination that the way back to WHOLE would complete
    members[1].set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    members[1].set_frame_mask(mask)
    members[1].set_direct_similarity(0.9)
    with pytest.raises(capi.SlideoError) as e:
        g.set_direct_scope(capi.DIRECT_WHOLE)
    assert e.value.code == 5 and scopes() == [capi.DIRECT_VALID] * 2
    members[1].set_direct_similarity(0.0)
    members[1].set_frame_mask(None)
    members[1].set_frame_mask_scope(capi.MASK_DETECT)
    # the last member alone busy
    d = torch.from_numpy(stream[0][:2]).cuda()
    tk = members[1].submit_changed_dev(d.data_ptr(), 2, W, H)
    with pytest.raises(capi.SlideoError) as e:
        g.set_direct_scope(capi.DIRECT_WHOLE)
    assert e.value.code == 4 and scopes() == [capi.DIRECT_VALID] * 2
    members[1].collect_changed(tk)
    members[1].gate_reset(None)
    g.set_direct_scope(capi.DIRECT_WHOLE)
    assert scopes() == [capi.DIRECT_WHOLE] * 2
    g.close()


# ---- 7. the setters ---------------------------------------------------------------------------------------------------------------

def _run(m, seq):
    out = m.match_changed_frames(seq)
    direct = (out[2]["page_idx"] >= 0) & (out[2]["inliers"] == 0)
    k = int((out[0] & ~direct).sum())
    res = [x.tobytes() for x in out] + [m.last_candidates(i).tobytes() for i in range(k)] + [m.gate_last_small().tobytes()]
    m.close()
    return res, direct


def test_valid_without_a_map_is_whole_bit_for_bit(capi, deck, taps, stream):
    """No mask, a mask under DETECT alone, and the all-255 mask under DETECT | GATE (against no mask under WHOLE)."""
    seq = stream[0][:10]
    hole, all255 = taps["A"]["masks"]["hole"][0], taps["A"]["masks"]["all"][0]
    t = 0.7
    whole, direct = _run(_matcher(capi, deck, scope=capi.DIRECT_WHOLE, t=t), seq)
    assert direct.any() and not direct.all()
    assert _run(_matcher(capi, deck, scope=capi.DIRECT_VALID, t=t), seq)[0] == whole
    assert _run(_matcher(capi, deck, mask=all255, mask_scope=capi.MASK_DETECT | capi.MASK_GATE, scope=capi.DIRECT_VALID, t=t), seq)[0] == whole
    det_whole, d2 = _run(_matcher(capi, deck, mask=hole, mask_scope=capi.MASK_DETECT, scope=capi.DIRECT_WHOLE, t=t), seq)
    assert d2.any()
    assert _run(_matcher(capi, deck, mask=hole, mask_scope=capi.MASK_DETECT, scope=capi.DIRECT_VALID, t=t), seq)[0] == det_whole


def test_setter_rules(capi, deck, taps, stream):
    import torch
    mask = taps["A"]["masks"]["hole"][0]
    both = capi.MASK_DETECT | capi.MASK_GATE
    m = _matcher(capi, deck)
    assert m.direct_scope == capi.DIRECT_WHOLE
    for bad in (2, 3, 0xFFFFFFFF):
        with pytest.raises(capi.SlideoError) as e:
            m.set_direct_scope(bad)
        assert e.value.code == 1 and m.direct_scope == capi.DIRECT_WHOLE
    # a busy matcher
    d = torch.from_numpy(stream[0][:2]).cuda()
    tk = m.submit_changed_dev(d.data_ptr(), 2, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_direct_scope(capi.DIRECT_VALID)
    assert e.value.code == 4 and m.direct_scope == capi.DIRECT_WHOLE
    m.collect_changed(tk)
    m.gate_reset(None)
    # under VALID none of the three set calls refuses, in any order
    m.set_direct_scope(capi.DIRECT_VALID)
    m.set_frame_mask_scope(both); m.set_frame_mask(mask); m.set_direct_similarity(0.9)
    m.set_frame_mask(None); m.set_frame_mask(mask)
    m.set_frame_mask_scope(capi.MASK_DETECT); m.set_frame_mask_scope(both)
    # the refused way back to WHOLE: the fourth set call that can complete the combination
    with pytest.raises(capi.SlideoError) as e:
        m.set_direct_scope(capi.DIRECT_WHOLE)
    assert e.value.code == 5 and m.direct_scope == capi.DIRECT_VALID and m.direct_similarity == np.float32(0.9)
    m.set_direct_similarity(0.0)
    m.set_direct_scope(capi.DIRECT_WHOLE)                           # t = 0: nothing to refuse
    m.set_direct_scope(capi.DIRECT_VALID); m.set_direct_similarity(0.9); m.set_frame_mask(None)
    m.set_direct_scope(capi.DIRECT_WHOLE)                           # no mask: nothing to refuse
    m.close()


def test_under_whole_the_refusal_is_still_raised_in_all_three_orders(capi, deck, taps):
    mask = taps["A"]["masks"]["hole"][0]
    both = capi.MASK_DETECT | capi.MASK_GATE
    m = _matcher(capi, deck)
    m.set_frame_mask_scope(both); m.set_frame_mask(mask)
    with pytest.raises(capi.SlideoError) as e:
        m.set_direct_similarity(0.9)
    assert e.value.code == 5 and m.direct_similarity == 0.0
    m.set_frame_mask(None)
    m.set_direct_similarity(0.9)
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask(mask)
    assert e.value.code == 5 and m.frame_mask_info is None
    m.set_frame_mask_scope(capi.MASK_DETECT)
    m.set_frame_mask(mask)
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask_scope(both)
    assert e.value.code == 5 and m.frame_mask_scope == capi.MASK_DETECT
    m.close()
