"""The gated calls under a gate settle (include/slideo_amd.h "Gate settle") against the definition: flags and similarities from the
numpy restatement (tests/gate_settle_ref.py) over small images from the shipped small-image tap, verdicts and traces from
match_frames of the matched frames on a second, ungated matcher, the last small image = the anchor's.  Every comparison is exact
equality of bytes; the gated path's own output is never the reference.

The stream (`_stream_frames`, 102 frames of 640x360): the 96 frames of tests/test_gpu_gate_anchor.py's stream, built here — holds,
hard cuts, a hold with three altered pixels per frame, a 24-step fade (frames 10 .. 38) and a second one (48 .. 76) inside which the
boundaries of 7- and 32-frame units fall (49, 56, 63, 64, 70), a long last hold — and a six-frame hold under +-3 noise (96 .. 101).
`_conditions` asserts on the restatement, before anything is compared, that the stream does what it was built for."""
import os

import numpy as np
import pytest

import gate_anchor_ref as aref
import gate_mask_ref as gref
import gate_settle_ref as sref
import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
W, H = 640, 360
CS = 0.98                                                        # slideo_config_default's changed_similarity
SETTLE = 0.99
NEVER = 2 ** 30
SETTLES = [(SETTLE, NEVER), (SETTLE, 4), (SETTLE, 0)]
UNCHANGED = (-1, 0.0, 0, 0)
UNITS = (1, 7, 32)
HOLE = (190, 350, 390, 630)
INSET = (191, 349, 391, 629)


def _fade(a, b, k):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return [a, a, a] + [np.rint(a64 + (b64 - a64) * j / k).astype(np.uint8) for j in range(1, k)] + [b, b, b]


def _stream_frames(base, full):
    """base: eight synthetic frames; full: two full-screen slide frames (a page reduced to the frame size)."""
    rng = np.random.default_rng(17)
    seq = [base[0]] * 5
    for _ in range(5):                                           # a hold of base[1] with three altered pixels per frame
        f = base[1].copy()
        f[rng.integers(0, H, 3), rng.integers(0, W, 3)] ^= 0x55
        seq.append(f)
    seq += _fade(base[1], base[2], 24)                           # 10 .. 38
    seq += [full[0]] * 6                                         # 39 .. 44: a hard cut to a full-screen slide
    seq += [base[4]] * 3                                         # 45 .. 47
    seq += _fade(base[5], base[6], 24)                           # 48 .. 76 (48: a hard cut)
    seq += [full[1]] * 8                                         # 77 .. 84
    seq += [base[7]] * 11                                        # 85 .. 95
    noise = np.random.default_rng(19)
    seq += [np.clip(base[3].astype(np.int16) + noise.integers(-3, 4, base[3].shape), 0, 255).astype(np.uint8) for _ in range(6)]      # 96 .. 101
    seq = np.stack(seq)
    assert len(seq) == 102
    return seq


def _conditions(smalls, settle, valid=None):
    """Conditions on the INPUT, by the restatements alone."""
    ach = aref.flags(smalls, valid, CS)[0]
    ch, sim, kind, d, state = sref.flags(smalls, valid, CS, settle[0], settle[1])
    n = len(smalls)
    if settle[1] == 0:
        assert np.array_equal(ch, ach), "a cap of 0 is the ANCHOR rule"
        return ch
    assert not np.array_equal(ch, ach) and ch.sum() < ach.sum(), "the settle's flags differ from ANCHOR's"
    assert (kind == sref.DEFERRED).any() and (kind == sref.MATCHED_STILL).any()
    assert (kind == sref.MATCHED_CAP).any() == (settle[1] != NEVER)
    last = np.maximum.accumulate(np.where(ch, np.arange(n), -1))  # the anchor behind frame i
    # (under a cap of 4 a fade is a period of six frames — one unchanged, four deferred, one matched by the cap —, so no 7-frame unit
    # is without a matched frame, and of this stream's 32-frame boundaries none happens to carry a count: those two are conditions
    # of the uncapped settle)
    for u in (7, 32):
        b = np.arange(u, n, u)
        if u == 7 or settle[1] == NEVER:
            assert (d[b] > 0).any(), "unit size %d: some unit boundary falls inside a run of deferred frames" % u
        assert (last[b - 1] != b - 1).any(), "unit size %d: at some unit boundary the previous frame is not the anchor" % u
    if settle[1] == NEVER:
        assert any((kind[lo:lo + 7] == sref.DEFERRED).any() and not ch[lo:lo + 7].any() for lo in range(0, n, 7)), \
            "a 7-frame unit with deferred frames and no matched one"
    return ch


def _matcher(capi, pages, settle=None, mask=None, t=None, anchor=True):
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    if mask is not None:
        m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        m.set_frame_mask(mask)
    if t is not None:
        if mask is not None:
            m.set_direct_scope(capi.DIRECT_VALID)
        m.set_direct_similarity(t)
    if anchor:
        m.set_gate_reference("anchor")
    if settle is not None:
        m.set_gate_settle(*settle)
        got = m.gate_settle()
        assert got == (float(np.float32(settle[0])), settle[1])
    return m


class Want:
    """The definition over `seq` from the state "none" or a carried state: flags and similarities from the restatement, verdicts and
    traces of the matched frames from match_frames on r (a matcher under the PREVIOUS default: a plain call does not look at the
    gate), the others — unchanged and deferred alike — (-1, 0, 0, 0) or, `direct` (frame -> verdict), the look-up's."""

    def __init__(self, capi, r, seq, smalls, settle, valid=None, state=None, direct=None, yuv=None):
        self.changed, self.sims, self.kind, self.d, self.state = sref.flags(smalls, valid, CS, settle[0], settle[1], state)
        direct = direct or {}
        self.v = np.zeros(len(seq), capi.VERDICT_DTYPE)
        self.v[:] = UNCHANGED
        self.pipe = np.array([i for i in np.nonzero(self.changed)[0] if i not in direct], np.int64)
        if len(self.pipe):
            self.v[self.pipe] = r.match_frames(seq[self.pipe]) if yuv is None else r.match_frames_yuv420(seq[self.pipe], *yuv)
        self.traces = [r.last_candidates(k).tobytes() for k in range(len(self.pipe))]
        for i in np.nonzero(self.changed)[0]:
            if i in direct:
                self.v[i] = direct[i]


def _equal(want, got, lo=0, hi=None, what=""):
    changed, sims, v = got
    hi = len(want.changed) if hi is None else hi
    assert len(changed) == hi - lo, what
    assert np.array_equal(changed, want.changed[lo:hi]), (what, "flags", np.nonzero(changed != want.changed[lo:hi])[0][:8] + lo)
    assert sims.tobytes() == want.sims[lo:hi].tobytes(), (what, "similarities", np.nonzero(sims != want.sims[lo:hi])[0][:8] + lo)
    assert v.tobytes() == want.v[lo:hi].tobytes(), (what, "verdicts", [i + lo for i in range(hi - lo) if v[i] != want.v[lo + i]][:8])


def _traces(want, m, what=""):
    for k, tr in enumerate(want.traces):
        assert m.last_candidates(k).tobytes() == tr, (what, "trace of pipeline frame %d" % k)


def _units(m, submit, n, unit):
    """Gated submit / collect in units of `unit`, max_in_flight at once, in order -> the concatenated result."""
    got, pend = [], []
    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            got.append(m.collect_changed(pend.pop(0)))
        pend.append(submit(i, min(unit, n - i)))
    got += [m.collect_changed(t) for t in pend]
    return tuple(np.concatenate([g[j] for g in got]) for j in range(3))


@pytest.fixture(scope="module")
def data(capi, synth):
    """-> pages, the stream, its small images (the shipped tap), the reference matcher r (PREVIOUS, no mask), the definition per
    settle value."""
    pages = synth.pages(4, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 8, W, H, threads=NCPU)
    r = _matcher(capi, pages, anchor=False)
    full = [r.reduce(pages[p], W, H) for p in (0, 3)]
    seq = _stream_frames(base, full)
    smalls = np.stack([r.small_image(f) for f in seq])
    assert smalls.shape[1:] == (259, 461, 3)
    wants = {}
    for settle in SETTLES:
        _conditions(smalls, settle)
        wants[settle] = Want(capi, r, seq, smalls, settle)
    # the noisy hold: matched once, on its second frame, and nothing in it is away after that
    w = wants[(SETTLE, NEVER)]
    assert np.nonzero(w.changed[96:])[0].tolist() == [1] and w.kind[96] == sref.DEFERRED and (w.kind[98:] == sref.UNCHANGED).all()
    yield pages, seq, smalls, r, wants
    r.close()


@pytest.mark.parametrize("settle", SETTLES)
def test_synchronous_host_and_device(capi, data, settle):
    import torch
    pages, seq, smalls, _, wants = data
    want = wants[settle]
    m = _matcher(capi, pages, settle)
    got = m.match_changed_frames(seq)
    _equal(want, got, what="host, one call")
    _traces(want, m, "host, one call")
    assert np.array_equal(m.gate_last_small(), want.state[0]), "the state is the anchor's small image"
    assert np.array_equal(capi.gate_deferred(got[0], got[1], CS), want.kind == sref.DEFERRED)
    # several calls continue anchor, previous frame and count: cuts inside both fades, a one-frame call, a call without a matched frame
    m.gate_reset(None)
    cuts = (0, 20, 21, 60, 88, 102)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _equal(want, m.match_changed_frames(seq[lo:hi]), lo, hi, "host call %d..%d" % (lo, hi))
        assert np.array_equal(m.gate_last_small(), smalls[np.nonzero(want.changed[:hi])[0].max()])
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    _equal(want, m.match_changed_frames_dev(d.data_ptr(), len(seq), W, H), what="device, one call")
    _traces(want, m, "device, one call")
    assert np.array_equal(m.gate_last_small(), want.state[0])
    m.close()


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("settle", SETTLES)
def test_submit_collect_units(capi, data, settle, unit):
    import torch
    pages, seq, _, _, wants = data
    want = wants[settle]
    n, fb = len(seq), W * H * 3
    d = torch.from_numpy(seq).cuda()
    m = _matcher(capi, pages, settle)
    assert m.max_in_flight() > 1
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H), n, unit)
    _equal(want, got, what="units of %d" % unit)
    _traces(want, m, "units of %d" % unit)
    assert np.array_equal(m.gate_last_small(), want.state[0])
    m.close()


@pytest.mark.parametrize("settle", SETTLES)
def test_nv12_device_units(capi, data, settle):
    """4:2:0 frames stand for their BGR image: the small images of the conversion tap's output."""
    import torch
    pages, seq, _, r, _ = data
    L, fb = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(seq, L, fb)
    smalls = np.stack([r.small_image(r.yuv420_to_bgr(f, W, H, L)) for f in yuv])
    _conditions(smalls, settle)
    want = Want(capi, r, yuv, smalls, settle, yuv=(W, H, L))
    d = torch.from_numpy(yuv).cuda()
    fs = yuv.shape[1]
    m = _matcher(capi, pages, settle)
    got = _units(m, lambda i, c: m.submit_changed_yuv420_dev(d.data_ptr() + i * fs, c, W, H, L, fs), len(yuv), 7)
    _equal(want, got, what="nv12 units of 7")
    assert np.array_equal(m.gate_last_small(), want.state[0])
    m.gate_reset(None)
    _equal(want, m.match_changed_frames_yuv420(yuv, W, H, L), what="nv12 host")
    m.close()


def test_a_cap_of_0_is_plain_anchor(capi, data):
    """(0.99, 0) against a matcher under plain ANCHOR, on every output, call by call."""
    pages, seq, _, _, _ = data
    a = _matcher(capi, pages)
    s = _matcher(capi, pages, (SETTLE, 0))
    for lo, hi in ((0, 20), (20, 21), (21, 60), (60, 102)):
        ga, gs = a.match_changed_frames(seq[lo:hi]), s.match_changed_frames(seq[lo:hi])
        for x, y in zip(ga, gs):
            assert x.tobytes() == y.tobytes()
        assert [a.last_candidates(k).tobytes() for k in range(int(ga[0].sum()))] == [s.last_candidates(k).tobytes() for k in range(int(gs[0].sum()))]
        assert np.array_equal(a.gate_last_small(), s.gate_last_small())
    a.close()
    s.close()


def test_a_starting_state_from_a_small_image_and_from_a_frame(capi, data):
    import torch
    pages, seq, smalls, r, wants = data
    settle = (SETTLE, NEVER)
    lo = 20                                                      # inside the first fade: anchor = previous = frame 19, nothing deferred
    want = Want(capi, r, seq[lo:], smalls[lo:], settle, state=(smalls[19], smalls[19], 0))
    assert want.kind[0] == sref.UNCHANGED and wants[settle].kind[lo] == sref.DEFERRED, "frame 20 is one step from frame 19: the carried state decides"
    assert (want.kind == sref.DEFERRED).any()
    m = _matcher(capi, pages, settle)
    m.gate_reset(smalls[19])
    assert np.array_equal(m.gate_last_small(), smalls[19])
    _equal(want, m.match_changed_frames(seq[lo:]), what="gate_reset(prev_small)")
    assert np.array_equal(m.gate_last_small(), want.state[0])
    m.gate_reset_from_frame(seq[19])
    assert np.array_equal(m.gate_last_small(), smalls[19])
    d = torch.from_numpy(seq[lo:]).cuda()
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(seq) - lo, 7)
    _equal(want, got, what="gate_reset_from_frame, units of 7")
    m.close()


def test_mask_gate_scope_with_an_inset_renewed_on_every_frame(capi, oracle, data):
    pages, seq, _, _, _ = data
    settle = (SETTLE, NEVER)
    mask = np.full((H, W), 255, np.uint8)
    mask[HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = 0
    rng = np.random.default_rng(23)
    ins = seq.copy()
    for f in ins:
        f[INSET[0]:INSET[1], INSET[2]:INSET[3]] = rng.integers(0, 256, (INSET[1] - INSET[0], INSET[3] - INSET[2], 3), dtype=np.uint8)
    valid, nv = gref.validity_map(oracle, mask)
    rm = _matcher(capi, pages, anchor=False, mask=mask)          # (verdicts of the matched frames under the same detection mask)
    smalls = np.stack([rm.small_image(f) for f in ins])
    _conditions(smalls, settle, valid)
    whole = sref.flags(smalls, None, CS, SETTLE, NEVER)
    assert whole[0].sum() == 1 and (whole[2][1:] == sref.DEFERRED).all(), "unmasked, the inset keeps every frame away and none still"
    want = Want(capi, rm, ins, smalls, settle, valid=valid)
    m = _matcher(capi, pages, settle, mask=mask)
    _equal(want, m.match_changed_frames(ins), what="mask, host")
    _traces(want, m, "mask, host")
    assert np.array_equal(m.gate_last_small(), want.state[0]), "the state is unmasked"
    import torch
    d = torch.from_numpy(ins).cuda()
    m.gate_reset(None)
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(ins), 7)
    _equal(want, got, what="mask, units of 7")
    m.close()
    rm.close()


def test_direct_similarity_sees_matched_frames_only(capi, data):
    pages, seq, smalls, r, wants = data
    settle = (SETTLE, NEVER)
    base = wants[settle]
    ssd = r.page_small_ssd(smalls).astype(np.int64)              # the shipped tap, on the reference matcher
    best = ssd.min(axis=1)
    page = ssd.argmin(axis=1)                                    # (the lowest page with the smallest SSD)
    sims = np.array([gref.similarity(int(b), 259 * 461) for b in best], np.float32)
    full = np.zeros(len(seq), bool)
    full[39:45] = True
    full[77:85] = True
    lo, hi = float(sims[~full].max()), float(sims[full].min())
    assert lo < hi, "the full-screen slide frames are closer to their page than any other frame to any"
    t = float(np.float32((lo + hi) / 2))
    direct = {int(i): (int(page[i]), sims[i], 0, 0) for i in np.nonzero(base.changed)[0] if sims[i] >= np.float32(t)}
    # a hard cut is matched on the second frame of the new hold: the look-up never sees the deferred first one
    assert sorted(direct) == [40, 78] and [direct[40][0], direct[78][0]] == [0, 3]
    assert base.kind[39] == sref.DEFERRED and base.kind[77] == sref.DEFERRED and sims[39] >= np.float32(t)
    want = Want(capi, r, seq, smalls, settle, direct=direct)
    assert np.array_equal(want.changed, base.changed) and len(want.pipe) == int(base.changed.sum()) - 2
    m = _matcher(capi, pages, settle, t=t)
    _equal(want, m.match_changed_frames(seq), what="direct, host")
    _traces(want, m, "direct, host")
    import torch
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(seq), 32)
    _equal(want, got, what="direct, units of 32")
    assert np.array_equal(m.gate_last_small(), want.state[0])
    m.close()


def test_groups(capi, data):
    pages, seq, _, _, wants = data
    settle = (SETTLE, NEVER)
    want = wants[settle]
    g = capi.Group(small_cfg(capi), devices=[0])
    g.add_pages(list(pages))
    g.finalize()
    g.set_gate_reference("anchor")
    g.set_gate_settle(*settle)
    assert g.gate_settle() == (float(np.float32(SETTLE)), NEVER)
    _equal(want, g.match_changed_frames(seq), what="group of one")
    _traces(want, g, "group of one")
    assert np.array_equal(g.gate_last_small(), want.state[0])
    g.close()
    g2 = capi.Group(small_cfg(capi), devices=[0, 0])
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_settle(*settle)
    assert e.value.code == 5 and "one member" in str(e.value)
    assert [g2.member(i).gate_settle() for i in range(2)] == [(0.0, 0), (0.0, 0)], "no member is changed"
    g2.set_gate_settle(0, 0)                                     # off: always accepted
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_settle(1.5, 0)
    assert e.value.code == 1
    g2.close()
    # the mirror: the refusal surfaces when the group is built
    from slideo_amd import matching
    with pytest.raises(capi.SlideoError) as e:
        matching.HipImageVideoMatcher(cfg=small_cfg(capi), devices=[0], gate_settle=settle).create_video_matcher(
            [], matching.ProgressReporter(lambda *a: None))
    assert e.value.code == 5, "a settle under the PREVIOUS default"


def test_setter_rules(capi, data):
    import torch
    pages, seq, smalls, _, _ = data
    m = _matcher(capi, pages, anchor=False)
    assert m.gate_settle() == (0.0, 0)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_settle(SETTLE, 4)
    assert e.value.code == 5 and "SLIDEO_GATE_ANCHOR" in str(e.value) and m.gate_settle() == (0.0, 0), "settle under PREVIOUS"
    m.set_gate_settle(0, 3)                                      # off is accepted under PREVIOUS
    m.set_gate_reference("anchor")
    for bad in ((-0.1, 0), (1.5, 0), (float("nan"), 0)):
        with pytest.raises(capi.SlideoError) as e:
            m.set_gate_settle(*bad)
        assert e.value.code == 1 and m.gate_settle() == (0.0, 3)
    assert capi.lib().slideo_matcher_set_gate_settle(m._h, 0.5, -1) == 1 and m.gate_settle() == (0.0, 3)
    m.set_gate_settle(SETTLE, 4)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_reference("previous")
    assert e.value.code == 5 and m.gate_reference() == "anchor" and m.gate_settle() == (float(np.float32(SETTLE)), 4), "PREVIOUS while settle is on"
    d = torch.from_numpy(seq[:4]).cuda()
    t = m.submit_changed_dev(d.data_ptr(), 4, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_settle(SETTLE, 5)
    assert e.value.code == 4 and m.gate_settle() == (float(np.float32(SETTLE)), 4), "the setter needs an idle matcher"
    m.collect_changed(t)
    assert np.array_equal(m.gate_last_small(), smalls[0])
    for settle in ((SETTLE, 4), (SETTLE, 4), (0, 0)):            # setting it resets the gate state, also to the values in force
        m.gate_reset(smalls[0])
        m.set_gate_settle(*settle)
        with pytest.raises(capi.SlideoError) as e:
            m.gate_last_small()
        assert e.value.code == 4
    m.set_gate_reference("previous")                             # settle is off: accepted
    m.close()
