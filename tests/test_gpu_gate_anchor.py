"""The gated calls under SLIDEO_GATE_ANCHOR (include/slideo_amd.h "Gate reference") against the definition: flags, similarities and the
anchor from the numpy restatement (tests/gate_anchor_ref.py) over small images from the shipped small-image tap, verdicts and traces
from match_frames of the flagged frames on a second matcher, the last small image = the anchor's.  Every comparison is exact
equality of bytes; the gated path's own output is never the reference.

The stream (`_stream_frames`, 96 frames of 640x360): holds, hard cuts, a hold with three altered pixels per frame, a 24-step fade
(frames 10 .. 38) and a second one (48 .. 76) inside which the boundaries of 7- and 32-frame units fall (49, 56, 63, 64, 70), and a
last hold long enough that a 7-frame unit holds no flagged frame.  `_conditions` asserts on the restatement, before anything is
compared, that the stream does what it was built for."""
import os

import numpy as np
import pytest

import gate_anchor_ref as aref
import gate_mask_ref as gref
import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
W, H = 640, 360
CS = 0.98                                                        # slideo_config_default's changed_similarity
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
    seq = np.stack(seq)
    assert len(seq) == 96
    return seq


def _conditions(smalls, valid=None):
    """Conditions on the INPUT, by the restatement alone."""
    prev, _ = gref.flags(smalls, valid, CS)
    ch, sim, ref, last = aref.flags(smalls, valid, CS)
    assert not np.array_equal(prev, ch), "the two rules differ on this stream"
    assert not prev[13:36].any() and ch[13:36].any() and not prev[51:74].any() and ch[51:74].any(), "the fades: PREVIOUS misses them, ANCHOR does not"
    n = len(smalls)
    for u in (7, 32):
        b = np.arange(u, n, u)
        assert (ref[b] != b - 1).any(), "unit size %d: at some unit boundary the anchor is not the frame before" % u
    assert any(not ch[lo:lo + 7].any() and ref[lo] < lo - 1 for lo in range(7, n, 7)), \
        "a 7-frame unit without a flagged frame whose carried anchor is older than the frame before the unit"
    assert any(ch[lo:lo + 7].sum() > 1 for lo in range(0, n, 7)), "a unit in which the anchor moves more than once"
    return ch, sim, ref, last


def _matcher(capi, pages, anchor=True, mask=None, t=None):
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
        assert m.gate_reference() == "anchor"
    return m


class Want:
    """The definition over `seq` from the state "none" or a carried anchor: flags and similarities from the restatement, verdicts and
    traces of the frames that go through the pipeline from match_frames on r (a matcher under the PREVIOUS default: a plain call
    does not look at the gate), the others (-1, 0, 0, 0) or, `direct` (frame -> verdict), the look-up's."""

    def __init__(self, capi, r, seq, smalls, valid=None, anchor_small=None, direct=None, yuv=None):
        self.changed, self.sims, self.ref, self.last = aref.flags(smalls, valid, CS, anchor_small)
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
    """-> pages, the stream, its small images (the shipped tap), the reference matcher r (PREVIOUS, no mask) and the definition."""
    pages = synth.pages(4, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 8, W, H, threads=NCPU)
    r = _matcher(capi, pages, anchor=False)
    full = [r.reduce(pages[p], W, H) for p in (0, 3)]
    seq = _stream_frames(base, full)
    smalls = np.stack([r.small_image(f) for f in seq])
    assert smalls.shape[1:] == (259, 461, 3)
    _conditions(smalls)
    want = Want(capi, r, seq, smalls)
    yield pages, seq, smalls, r, want
    r.close()


def test_synchronous_host_and_device(capi, data):
    import torch
    pages, seq, smalls, _, want = data
    m = _matcher(capi, pages)
    _equal(want, m.match_changed_frames(seq), what="host, one call")
    _traces(want, m, "host, one call")
    assert np.array_equal(m.gate_last_small(), want.last), "the state is the anchor's small image"
    # several calls continue the anchor: cuts inside both fades, a one-frame call, a call without a flagged frame
    m.gate_reset(None)
    cuts = (0, 20, 21, 60, 88, 96)
    assert not want.changed[88:].any()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _equal(want, m.match_changed_frames(seq[lo:hi]), lo, hi, "host call %d..%d" % (lo, hi))
        assert np.array_equal(m.gate_last_small(), smalls[np.nonzero(want.changed[:hi])[0].max()])
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    _equal(want, m.match_changed_frames_dev(d.data_ptr(), len(seq), W, H), what="device, one call")
    _traces(want, m, "device, one call")
    assert np.array_equal(m.gate_last_small(), want.last)
    m.close()


@pytest.mark.parametrize("unit", UNITS)
def test_submit_collect_units(capi, data, unit):
    import torch
    pages, seq, _, _, want = data
    n, fb = len(seq), W * H * 3
    d = torch.from_numpy(seq).cuda()
    m = _matcher(capi, pages)
    assert m.max_in_flight() > 1
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H), n, unit)
    _equal(want, got, what="units of %d" % unit)
    _traces(want, m, "units of %d" % unit)
    assert np.array_equal(m.gate_last_small(), want.last)
    m.close()


def test_nv12_device_units(capi, data):
    """4:2:0 frames stand for their BGR image: the small images of the conversion tap's output."""
    import torch
    pages, seq, _, r, _ = data
    L, fb = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(seq, L, fb)
    smalls = np.stack([r.small_image(r.yuv420_to_bgr(f, W, H, L)) for f in yuv])
    _conditions(smalls)
    want = Want(capi, r, yuv, smalls, yuv=(W, H, L))
    d = torch.from_numpy(yuv).cuda()
    fs = yuv.shape[1]
    m = _matcher(capi, pages)
    got = _units(m, lambda i, c: m.submit_changed_yuv420_dev(d.data_ptr() + i * fs, c, W, H, L, fs), len(yuv), 7)
    _equal(want, got, what="nv12 units of 7")
    assert np.array_equal(m.gate_last_small(), want.last)
    m.gate_reset(None)
    _equal(want, m.match_changed_frames_yuv420(yuv, W, H, L), what="nv12 host")
    m.close()


def test_a_starting_anchor_from_a_small_image_and_from_a_frame(capi, data):
    import torch
    pages, seq, smalls, r, _ = data
    lo = 20                                                      # inside the first fade, from an anchor the whole stream never had
    start = seq[19]
    assert not data[4].changed[19] and data[4].changed[20]
    want = Want(capi, r, seq[lo:], smalls[lo:], anchor_small=smalls[19])
    assert want.ref[0] == -1 and not want.changed[0] and want.changed[1], "frame 20 is one step from frame 19: the carried anchor decides"
    m = _matcher(capi, pages)
    m.gate_reset(smalls[19])
    assert np.array_equal(m.gate_last_small(), smalls[19])
    _equal(want, m.match_changed_frames(seq[lo:]), what="gate_reset(prev_small)")
    assert np.array_equal(m.gate_last_small(), want.last)
    m.gate_reset_from_frame(start)
    assert np.array_equal(m.gate_last_small(), smalls[19])
    d = torch.from_numpy(seq[lo:]).cuda()
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(seq) - lo, 7)
    _equal(want, got, what="gate_reset_from_frame, units of 7")
    m.close()


def test_mask_gate_scope_with_an_inset_renewed_on_every_frame(capi, oracle, data):
    pages, seq, _, _, _ = data
    mask = np.full((H, W), 255, np.uint8)
    mask[HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = 0
    rng = np.random.default_rng(23)
    ins = seq.copy()
    for f in ins:
        f[INSET[0]:INSET[1], INSET[2]:INSET[3]] = rng.integers(0, 256, (INSET[1] - INSET[0], INSET[3] - INSET[2], 3), dtype=np.uint8)
    valid, nv = gref.validity_map(oracle, mask)
    rm = _matcher(capi, pages, anchor=False, mask=mask)          # (verdicts of the flagged frames under the same detection mask)
    smalls = np.stack([rm.small_image(f) for f in ins])
    ch, _, _, _ = _conditions(smalls, valid)
    assert aref.flags(smalls, None, CS)[0].all(), "unmasked, the inset flags every frame"
    assert not ch.all()
    want = Want(capi, rm, ins, smalls, valid=valid)
    m = _matcher(capi, pages, mask=mask)
    got_valid, got_n = m.frame_mask_small()
    assert np.array_equal(got_valid, valid) and got_n == nv
    _equal(want, m.match_changed_frames(ins), what="mask, host")
    _traces(want, m, "mask, host")
    assert np.array_equal(m.gate_last_small(), want.last), "the state is unmasked"
    import torch
    d = torch.from_numpy(ins).cuda()
    m.gate_reset(None)
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(ins), 7)
    _equal(want, got, what="mask, units of 7")
    m.close()
    rm.close()


def test_direct_similarity_held_to_the_page_tap(capi, data):
    pages, seq, smalls, r, base = data
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
    assert sorted(direct) == [39, 77] and [direct[39][0], direct[77][0]] == [0, 3]
    want = Want(capi, r, seq, smalls, direct=direct)
    assert np.array_equal(want.changed, base.changed) and len(want.pipe) == int(base.changed.sum()) - 2
    m = _matcher(capi, pages, t=t)
    _equal(want, m.match_changed_frames(seq), what="direct, host")
    _traces(want, m, "direct, host")
    import torch
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    got = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(seq), 32)
    _equal(want, got, what="direct, units of 32")
    assert np.array_equal(m.gate_last_small(), want.last)
    m.close()


def test_groups(capi, data):
    pages, seq, _, _, want = data
    g = capi.Group(small_cfg(capi), devices=[0])
    g.add_pages(list(pages))
    g.finalize()
    g.set_gate_reference("anchor")
    assert g.gate_reference() == "anchor"
    _equal(want, g.match_changed_frames(seq), what="group of one")
    _traces(want, g, "group of one")
    assert np.array_equal(g.gate_last_small(), want.last)
    g.close()
    g2 = capi.Group(small_cfg(capi), devices=[0, 0])
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_reference("anchor")
    assert e.value.code == 5 and "one member" in str(e.value)
    assert [g2.member(i).gate_reference() for i in range(2)] == ["previous", "previous"], "no member is changed"
    g2.set_gate_reference("previous")                            # always accepted
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_reference(7)
    assert e.value.code == 1
    g2.close()
    # the mirror: the refusal surfaces when the group is built
    from slideo_amd import matching
    with pytest.raises(capi.SlideoError) as e:
        matching.HipImageVideoMatcher(cfg=small_cfg(capi), devices=[0, 0], gate_reference="anchor").create_video_matcher(
            [], matching.ProgressReporter(lambda *a: None))
    assert e.value.code == 5


def test_setter_rules(capi, data):
    import torch
    pages, seq, smalls, _, _ = data
    m = _matcher(capi, pages, anchor=False)
    assert m.gate_reference() == "previous"
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_reference(2)
    assert e.value.code == 1 and m.gate_reference() == "previous"
    d = torch.from_numpy(seq[:4]).cuda()
    t = m.submit_changed_dev(d.data_ptr(), 4, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_reference("anchor")
    assert e.value.code == 4 and m.gate_reference() == "previous", "the setter needs an idle matcher"
    m.collect_changed(t)
    assert np.array_equal(m.gate_last_small(), smalls[3])
    for ref in ("anchor", "anchor", "previous"):                 # setting it resets the gate state, also to the value in force
        m.gate_reset(smalls[0])
        m.set_gate_reference(ref)
        assert m.gate_reference() == ref
        with pytest.raises(capi.SlideoError) as e:
            m.gate_last_small()
        assert e.value.code == 4
    m.close()


def test_default_after_setting_and_unsetting(capi, data):
    """Under PREVIOUS, after ANCHOR was set and unset, a gated call equals the existing mask + kept pair."""
    pages, seq, _, r, want = data
    changed, sims, last = r.changed_mask(seq)
    idx = np.nonzero(changed)[0]
    v = np.zeros(len(seq), capi.VERDICT_DTYPE)
    v[:] = UNCHANGED
    v[idx] = r.match_frames(seq[idx])
    assert not np.array_equal(changed, want.changed)
    m = _matcher(capi, pages)
    m.match_changed_frames(seq[:9])
    m.set_gate_reference("previous")
    got = m.match_changed_frames(seq)
    assert np.array_equal(got[0], changed) and got[1].tobytes() == sims.tobytes() and got[2].tobytes() == v.tobytes()
    assert np.array_equal(m.gate_last_small(), last)
    m.close()
