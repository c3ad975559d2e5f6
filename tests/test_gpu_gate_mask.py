"""Frame mask scope (include/slideo_amd.h "Frame mask scope") on the GPU: the validity map against its definition, the masked
flags and similarities of every call that makes them against ONE numpy restatement (tests/gate_mask_ref.py, over the CPU
to_small_image), the integer threshold at its edge, every byte alignment of the small images, and the scope's lifetime."""
import ctypes as C

import numpy as np
import pytest

import gate_mask_ref as gref
import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

W, H = 640, 360
HOLE = (190, 350, 390, 630)            # rows, columns of the hole in the 640x360 mask
INSET = (191, 349, 391, 629)           # the inset: one pixel inside the hole on every side
SIM = 0.98                             # slideo_config_default's changed_similarity


def _rect_hole(h, w, y0, y1, x0, x1):
    m = np.full((h, w), 255, np.uint8)
    m[y0:y1, x0:x1] = 0
    return m


def _with_inset(frames, seed):
    rng = np.random.default_rng(seed)
    out = frames.copy()
    y0, y1, x0, x1 = INSET
    for f in out:
        f[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0, 3), dtype=np.uint8)
    return out


def _deck(capi, pages, scope=None, mask=None):
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    if scope is not None:
        m.set_frame_mask_scope(scope)
    if mask is not None:
        m.set_frame_mask(mask)
    return m


@pytest.fixture(scope="module")
def content(capi, oracle, cfg0_data):
    """cfg0's frames with runs of held frames (each repeated 2 - 4 times), the same with an inset re-randomised on every frame, the
    hole mask, its validity map and the small images of both (CPU), computed once."""
    pages, frames, _, _ = cfg0_data
    assert capi.default_config().changed_similarity == np.float32(SIM)
    reps = [2, 3, 4, 2, 3, 4, 2, 3]
    seq = np.ascontiguousarray(np.repeat(frames, reps, axis=0))
    held = np.ones(len(seq), bool)
    held[np.cumsum([0] + reps[:-1])] = False
    ins = _with_inset(seq, 5)
    mask = _rect_hole(H, W, *HOLE)
    valid, n_valid = gref.validity_map(oracle, mask)
    return dict(pages=pages, seq=seq, ins=ins, held=held, mask=mask, valid=valid, n_valid=n_valid,
                s_seq=gref.small_images(oracle, seq), s_ins=gref.small_images(oracle, ins))


@pytest.fixture(scope="module")
def gm(capi, content):
    """cfg0's pages in a finalized matcher under DETECT | GATE with the hole mask."""
    m = _deck(capi, content["pages"], capi.MASK_DETECT | capi.MASK_GATE, content["mask"])
    yield m
    m.close()


def _eq(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert got[1].tobytes() == np.asarray(want[1], np.float32).tobytes(), (what, got[1], want[1])


# ---- 1. the map equals its definition ------------------------------------------------------------------------------------------

def _map_masks(h, w):
    rng = np.random.default_rng(h * 4099 + w)
    one = np.full((h, w), 255, np.uint8)
    one[h // 2 + 1, w // 3] = 0
    borders = np.full((h, w), 255, np.uint8)
    borders[:3, 40:90] = 0; borders[h - 2:, 100:107] = 0; borders[50:61, :5] = 0; borders[70:75, w - 1:] = 0
    borders[h - 9:, w - 11:] = 0                                    # a corner
    mixed = _rect_hole(h, w, h // 4, h // 2, w // 4, w // 2)
    mixed[mixed != 0] = rng.choice(np.array([1, 255], np.uint8), int((mixed != 0).sum()))      # nonzero is nonzero
    return {"rect": _rect_hole(h, w, h // 3 + 1, h - 7, w // 5 + 2, w - 13), "one": one, "borders": borders, "mixed": mixed}


@pytest.mark.parametrize("h,w,cases", [(360, 640, None), (300, 400, ("rect", "mixed")), (347, 349, ("rect", "borders")),
                                       (1080, 1920, ("borders",))])
def test_map_equals_its_definition(capi, oracle, h, w, cases):
    m = capi.Matcher(small_cfg(capi))
    m.set_frame_mask_scope(capi.MASK_GATE)
    L = capi.lib()
    seen_partial = False
    for name, mask in _map_masks(h, w).items():
        if cases and name not in cases:
            continue
        want, n = gref.validity_map(oracle, mask)
        m.set_frame_mask(mask)
        got, gn = m.frame_mask_small()
        assert got.shape == want.shape and gn == n == int(got.sum()), (name, gn, n)
        assert np.array_equal(got, want), "%s %dx%d: %d px differ" % (name, w, h, (got != want).sum())
        seen_partial |= 0 < n < want.size
        if (h, w) == (300, 400):                                     # the small image is the image itself
            assert np.array_equal(want, mask != 0)
        if name == "rect":                                           # the same mask given with a padded stride
            pad = np.zeros((h, w + 37), np.uint8)
            pad[:, :w] = mask
            pad[:, w:] = 77
            assert L.slideo_matcher_set_frame_mask(m._h, pad.ctypes.data, w, h, w + 37) == 0
            got2, gn2 = m.frame_mask_small()
            assert np.array_equal(got2, want) and gn2 == n
    assert seen_partial
    if (h, w) == (360, 640):
        # no small pixel is valid: refused, and the mask and scope before stay in force
        before, bn = m.frame_mask_small()
        cols = np.full((h, w), 255, np.uint8)
        cols[:, ::2] = 0
        assert gref.validity_map(oracle, cols)[1] == 0
        with pytest.raises(capi.SlideoError) as e:
            m.set_frame_mask(cols)
        assert e.value.code == 1 and "valid" in str(e.value)
        after, an = m.frame_mask_small()
        assert np.array_equal(before, after) and an == bn and m.frame_mask_scope == capi.MASK_GATE
        assert m.frame_mask_info == (w, h)
        # ... and the same refusal when the scope is the second of the two to arrive
        m.set_frame_mask_scope(capi.MASK_DETECT)
        m.set_frame_mask(cols)
        with pytest.raises(capi.SlideoError) as e:
            m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        assert e.value.code == 1 and m.frame_mask_scope == capi.MASK_DETECT
        # the sizes alone, and a capacity too small
        m.set_frame_mask(_rect_hole(h, w, 10, 20, 10, 20)); m.set_frame_mask_scope(capi.MASK_GATE)
        sw, sh, nv = C.c_int32(), C.c_int32(), C.c_int64()
        buf = np.zeros(16, np.uint8)
        assert L.slideo_frame_mask_small(m._h, buf.ctypes.data, C.c_int64(16), C.byref(sw), C.byref(sh), C.byref(nv)) == 7
        assert (sw.value, sh.value) == (461, 259) and nv.value > 0
        assert L.slideo_frame_mask_small(m._h, None, C.c_int64(0), None, C.byref(sh), C.byref(nv)) == 1
    m.close()


# ---- 2. all 255 is no mask -----------------------------------------------------------------------------------------------------

def test_all_255_under_gate_is_no_mask(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    m = _deck(capi, pages)
    ref_mask = m.changed_mask(frames)
    m.gate_reset(None)
    ref_gated = m.match_changed_frames(frames)
    ref_last = m.gate_last_small()
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(np.full((H, W), 255, np.uint8))
    assert m.frame_mask_small()[1] == 461 * 259
    got = m.changed_mask(frames)
    for a, b in zip(got, ref_mask):
        assert a.tobytes() == b.tobytes()
    m.gate_reset(None)
    got = m.match_changed_frames(frames)
    for a, b in zip(got, ref_gated):
        assert a.tobytes() == b.tobytes()
    assert m.gate_last_small().tobytes() == ref_last.tobytes()
    m.close()


# ---- 3. the definition, on content that needs it -------------------------------------------------------------------------------

def test_definition_on_frames_with_a_moving_inset(capi, content, gm):
    c = content
    want = gref.flags(c["s_ins"], c["valid"], SIM)
    assert np.array_equal(want[0], gref.flags(c["s_seq"], c["valid"], SIM)[0])
    assert want[1].tobytes() == gref.flags(c["s_seq"], c["valid"], SIM)[1].tobytes()      # no valid small pixel has an inset tap
    whole = gref.flags(c["s_ins"], None, SIM)
    assert (want[0][c["held"]] != whole[0][c["held"]]).any()         # a held frame the two scopes decide differently
    assert not want[0][c["held"]].any() and whole[0].all()           # (the inset defeats the unmasked gate on every frame here)
    gm.gate_reset(None)
    got = gm.match_changed_frames(c["ins"])
    _eq(got, want, "gated, inset")
    gm.gate_reset(None)
    clean = gm.match_changed_frames(c["seq"])
    _eq(clean, want, "gated, no inset")
    _eq(gm.changed_mask(c["ins"]), want, "mask call, inset")
    _eq(gm.changed_mask(c["seq"]), want, "mask call, no inset")
    # small images are never masked: the state is the last frame's whole small image
    assert np.array_equal(gm.gate_last_small(), c["s_seq"][-1])
    assert np.array_equal(gm.changed_mask(c["ins"])[2], c["s_ins"][-1])
    # DETECT only: today's unmasked flags
    gm.set_frame_mask_scope(capi.MASK_DETECT)
    try:
        gm.gate_reset(None)
        _eq(gm.match_changed_frames(c["ins"]), whole, "DETECT only, gated")
        _eq(gm.changed_mask(c["ins"]), whole, "DETECT only, mask call")
    finally:
        gm.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        gm.gate_reset(None)


# ---- 4. the threshold edge, exactly --------------------------------------------------------------------------------------------

def _squares(total):
    """Byte deltas (each <= 100) whose squares sum to exactly `total`."""
    out = [100] * (total // 10000)
    r = total % 10000
    while r > 0:
        d = int(np.floor(np.sqrt(r)))
        out.append(d)
        r -= d * d
    assert sum(d * d for d in out) == total
    return out


def test_threshold_edge(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    h, w = 300, 400                                                  # small_area pixels: the small image is the frame
    a = np.ascontiguousarray(frames[0][:h, :w])
    mask = _rect_hole(h, w, 40, 90, 300, 380)
    m = _deck(capi, pages, capi.MASK_DETECT | capi.MASK_GATE, mask)
    valid, n_valid = m.frame_mask_small()
    assert np.array_equal(valid, mask != 0) and n_valid == h * w - 50 * 80
    t = capi.changed_ssd_threshold_n(SIM, n_valid)
    assert t == gref.threshold(SIM, n_valid) and 0 < t
    rng = np.random.default_rng(17)
    pos = np.flatnonzero(np.repeat(valid[:, :, None], 3, axis=2).reshape(-1))

    def other(total):
        b = a.copy()
        b[40:90, 300:380] = rng.integers(0, 256, (50, 80, 3), dtype=np.uint8)     # arbitrary under the hole
        flat = b.reshape(-1)
        ds = _squares(total)
        at = rng.choice(pos, len(ds), replace=False)
        for p, d in zip(at, ds):
            flat[p] = flat[p] - d if flat[p] >= 100 else flat[p] + d
        assert gref.masked_ssd(a, b, valid) == total
        return b

    for total, flag in ((t - 1, False), (t, True), (0, False)):
        pair = np.stack([a, other(total)])
        sim = gref.similarity(total, n_valid)
        ch, s, _ = m.changed_mask(pair)
        assert bool(ch[1]) is flag and s[1].tobytes() == sim.tobytes(), (total, ch, s, sim)
        m.gate_reset(None)
        ch, s, _ = m.match_changed_frames(pair)
        assert bool(ch[1]) is flag and s[1].tobytes() == sim.tobytes() and ch[0] and s[0] == 0.0, (total, ch, s, sim)
        if total == 0:
            assert s[1] == np.float32(1.0)                           # differences under the hole alone
    m.close()


# ---- 5. alignment --------------------------------------------------------------------------------------------------------------

def test_every_alignment_and_odd_unit_boundaries(capi, content, gm):
    import torch
    c = content
    assert (461 * 259 * 3) % 4 == 1 and len(c["ins"]) >= 9            # consecutive small images start at every residue mod 4
    t = torch.from_numpy(c["ins"]).cuda()
    fb = W * H * 3
    want = gref.flags(c["s_ins"][1:10], c["valid"], SIM)
    gm.gate_reset(None)
    tk = [gm.submit_changed_dev(t.data_ptr() + 1 * fb, 1, W, H), gm.submit_changed_dev(t.data_ptr() + 2 * fb, 2, W, H),
          gm.submit_changed_dev(t.data_ptr() + 4 * fb, 6, W, H)]
    parts = [gm.collect_changed(x) for x in tk]
    _eq((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want, "units 1, 2, 6")
    # the whole sequence in one device call, the state carried on from the units
    got = gm.match_changed_frames_dev(t.data_ptr() + 10 * fb, len(c["ins"]) - 10, W, H)
    _eq(got, gref.flags(c["s_ins"][10:], c["valid"], SIM, prev_small=c["s_ins"][9]), "device call behind the units")
    gm.gate_reset(None)


# ---- 6. every path agrees with the one restatement -----------------------------------------------------------------------------

def test_nv12(capi, oracle, content, gm):
    c = content
    L, fbytes = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(c["ins"][:7], L, fbytes)
    conv = np.stack([gm.yuv420_to_bgr(y, W, H, L) for y in yuv])
    want = gref.flags(gref.small_images(oracle, conv), c["valid"], SIM)
    assert want[0].sum() >= 2 and not want[0].all()
    gm.gate_reset(None)
    _eq(gm.match_changed_frames_yuv420(yuv, W, H, L), want, "nv12 gated")
    _eq(gm.changed_mask_yuv420(yuv, W, H, L), want, "nv12 mask call")
    gm.gate_reset(None)


def test_working_size(capi, content, gm):
    c = content
    big = np.ascontiguousarray(c["ins"][:6].repeat(2, axis=1).repeat(2, axis=2))      # its 2x2 INTER_AREA reduction is the frames again
    want = gref.flags(c["s_ins"][:6], c["valid"], SIM)
    gm.set_working_size(W, H)
    try:
        _eq(gm.match_changed_frames(big), want, "working size, gated")
        _eq(gm.changed_mask(big), want, "working size, mask call")
        # the mask at the SOURCE size: the frames are analysed at 640x360, not the mask's size
        gm.set_frame_mask(np.full((2 * H, 2 * W), 255, np.uint8))
        for call in (gm.changed_mask, gm.match_changed_frames):
            with pytest.raises(capi.SlideoError) as e:
                call(big)
            assert e.value.code == 1 and "640x360" in str(e.value) and "1280x720" in str(e.value)
    finally:
        gm.set_frame_mask(c["mask"])
        gm.set_working_size(0, 0)
    with pytest.raises(capi.SlideoError) as e:                        # no working size: 1280x720 frames under the 640x360 mask
        gm.changed_mask(big)
    assert e.value.code == 1 and "640x360" in str(e.value) and "1280x720" in str(e.value)


def test_resets_and_the_chained_mask_call(capi, content, gm):
    c = content
    ins, s_ins = c["ins"][:12], c["s_ins"][:12]
    want = gref.flags(s_ins[1:], c["valid"], SIM, prev_small=s_ins[0])
    gm.gate_reset(s_ins[0])
    _eq(gm.match_changed_frames(ins[1:]), want, "gate_reset(prev_small)")
    gm.gate_reset_from_frame(ins[0])
    assert np.array_equal(gm.gate_last_small(), s_ins[0])
    _eq(gm.match_changed_frames(ins[1:]), want, "gate_reset_from_frame")
    gm.gate_reset(None)
    # the mask call chained over two calls, then the kept frames
    whole = gref.flags(s_ins, c["valid"], SIM)
    c1, s1, last = gm.changed_mask(ins[:5])
    c2, s2, _ = gm.changed_mask(ins[5:], prev_small=last)
    _eq((np.concatenate([c1, c2]), np.concatenate([s1, s2])), whole, "chained mask calls")
    idx = np.flatnonzero(c2)
    assert len(idx) >= 2
    kept = gm.match_kept_frames(idx)
    assert kept.tobytes() == gm.match_frames(ins[5:][idx]).tobytes()


@pytest.mark.parametrize("members", [2, 3])
def test_group_equals_the_single_matcher(capi, content, gm, members):
    c = content
    g = capi.Group(small_cfg(capi), devices=[0] * members)
    g.add_pages(list(c["pages"])); g.finalize()
    g.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    g.set_frame_mask(c["mask"])
    assert g.frame_mask_scope == 3 and g.member(members - 1).frame_mask_scope == 3
    assert g.frame_mask_small()[1] == c["n_valid"]
    for lo, hi in ((0, 11), (11, 13)):                               # the second call: fewer frames than members (3), state carried
        frames = c["ins"][lo:hi]
        if lo == 0:
            g.gate_reset(None); gm.gate_reset(None)
        want = gm.match_changed_frames(frames)
        traces = [gm.last_candidates(k) for k in range(int(want[0].sum()))]
        got = g.match_changed_frames(frames)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), (lo, hi)
        _eq(got, gref.flags(c["s_ins"][lo:hi], c["valid"], SIM, prev_small=c["s_ins"][lo - 1] if lo else None), "group")
        for k, tr in enumerate(traces):
            assert g.last_candidates(k).tobytes() == tr.tobytes(), (lo, k)
        assert g.gate_last_small().tobytes() == gm.gate_last_small().tobytes()
    _eq(g.changed_mask(c["ins"][:11]), gref.flags(c["s_ins"][:11], c["valid"], SIM), "group mask call")
    with pytest.raises(capi.SlideoError) as e:
        g.changed_mask(c["ins"][:4, :200])
    assert e.value.code == 1
    gm.gate_reset(None)
    g.close()


# ---- 7. scope and lifetime -----------------------------------------------------------------------------------------------------

def test_scope_and_lifetime(capi, content):
    import torch
    c = content
    ins, seq = c["ins"][:9], c["seq"][:9]
    masked = gref.flags(c["s_ins"][:9], c["valid"], SIM)
    whole = gref.flags(c["s_ins"][:9], None, SIM)
    plain = _deck(capi, c["pages"])
    assert plain.frame_mask_scope == capi.MASK_DETECT                  # the default
    with pytest.raises(capi.SlideoError) as e:                        # no mask: no map
        plain.frame_mask_small()
    assert e.value.code == 4
    # the scope after the mask
    m = _deck(capi, c["pages"], None, c["mask"])
    with pytest.raises(capi.SlideoError) as e:                        # a mask, but no GATE bit
        m.frame_mask_small()
    assert e.value.code == 4
    _eq(m.changed_mask(ins), whole, "default scope")
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    assert m.frame_mask_scope == 3
    assert np.array_equal(m.frame_mask_small()[0], c["valid"])
    _eq(m.changed_mask(ins), masked, "scope after the mask")
    for bad in (0, 4, 7):
        with pytest.raises(capi.SlideoError) as e:
            m.set_frame_mask_scope(bad)
        assert e.value.code == 1 and m.frame_mask_scope == 3
    # a scope change ends the kept frames and leaves the gate state
    m.gate_reset(None)
    m.match_changed_frames(ins[:3])
    state = m.gate_last_small()
    m.changed_mask(ins[:3])
    m.set_frame_mask_scope(capi.MASK_GATE)
    assert m.gate_last_small().tobytes() == state.tobytes()
    with pytest.raises(capi.SlideoError) as e:
        m.match_kept_frames(np.arange(2))
    assert e.value.code == 4
    # GATE only: keypoints and verdicts are the unmasked matcher's, the flags are the masked ones
    kp, desc = m.orb(seq[0])
    pk, pd = plain.orb(seq[0])
    assert kp.tobytes() == pk.tobytes() and np.array_equal(desc, pd)
    m.gate_reset(None); plain.gate_reset(None)
    got = m.match_changed_frames(ins)
    _eq(got, masked, "GATE only")
    idx = np.flatnonzero(masked[0])
    assert len(idx) >= 2 and got[2][idx].tobytes() == plain.match_frames(ins[idx]).tobytes()
    with pytest.raises(capi.SlideoError) as e:                        # the size rule holds under either bit
        m.match_frames(ins[:, :200])
    assert e.value.code == 1
    # a busy matcher
    t = torch.from_numpy(seq).cuda()
    tk = m.submit_dev(t.data_ptr(), 2, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_frame_mask_scope(capi.MASK_DETECT)
    assert e.value.code == 4 and m.frame_mask_scope == capi.MASK_GATE
    m.collect(tk)
    # the scope survives clearing the mask and is inert without one
    m.set_frame_mask(None)
    assert m.frame_mask_scope == capi.MASK_GATE
    m.gate_reset(None); plain.gate_reset(None)
    a, b = m.match_changed_frames(ins), plain.match_changed_frames(ins)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    _eq(a, whole, "no mask")
    # the scope before the mask
    m.set_frame_mask(c["mask"])
    assert np.array_equal(m.frame_mask_small()[0], c["valid"])
    _eq(m.changed_mask(ins), masked, "scope before the mask")
    m.close(); plain.close()
