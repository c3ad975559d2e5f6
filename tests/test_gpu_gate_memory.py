"""The gated calls under a gate memory (include/slideo_amd.h "Gate memory") against the definition: flags, similarities and refs from
the numpy restatement (tests/gate_memory_ref.py) over small images from the shipped small-image tap, verdicts and traces of the
matched frames from match_frames on a second, ungated matcher.  Every comparison is exact equality of bytes; the gated path's own
output is never the reference.

The stream (`_stream_frames`, 100 frames of 640x360) is a "revisit" lecture: holds of A, B, back to A, C, back to B, a hold of D under
+-3 noise, a full-screen slide F, E, back to the noisy D after those two holds, back to A, a return from A to C over a 24-step fade
(frames 42 .. 70, inside which the boundaries of 7- and 32-frame units fall: 49, 56, 63, 64, 70), a second full-screen slide G, back
to C, H, back to G, B, P, a flip to H and back to P, A.  `_conditions` asserts on the restatement, before anything is compared, that the stream does what it
was built for."""
import os

import numpy as np
import pytest

import gate_mask_ref as gref
import gate_memory_ref as mref
import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

NCPU = min(16, os.cpu_count() or 1)
W, H = 640, 360
CS = 0.98                                                        # slideo_config_default's changed_similarity
SETTLE = 0.99
NEVER = 2 ** 30
SETTLES = [None, (SETTLE, NEVER), (SETTLE, 4)]
MS = [1, 2, 4, 64]
UNCHANGED = (-1, 0.0, 0, 0)
HOLE = (190, 350, 390, 630)
INSET = (191, 349, 391, 629)


def _fade(a, b, k):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return [a, a, a] + [np.rint(a64 + (b64 - a64) * j / k).astype(np.uint8) for j in range(1, k)] + [b, b, b]


def _stream_frames(base, full):
    """base: eight synthetic frames; full: two full-screen slide frames (a page reduced to the frame size)."""
    A, B, Cc, D, E, Hh, P = base[0], base[1], base[2], base[3], base[4], base[5], base[6]
    noise = np.random.default_rng(19)

    def noisy(n):
        return [np.clip(D.astype(np.int16) + noise.integers(-3, 4, D.shape), 0, 255).astype(np.uint8) for _ in range(n)]

    seq = [A] * 5 + [B] * 5 + [A] * 3 + [Cc] * 5 + [B] * 3       # 0 .. 20
    seq += noisy(6)                                              # 21 .. 26
    seq += [full[0]] * 4 + [E] * 4                               # 27 .. 34
    seq += noisy(4)                                              # 35 .. 38: back to D after two other holds
    seq += [A] * 3                                               # 39 .. 41
    seq += _fade(A, Cc, 24)                                      # 42 .. 70: back to C over a fade
    seq += [full[1]] * 6 + [Cc] * 3 + [Hh] * 5 + [full[1]] * 3   # 71 .. 87
    seq += [B] * 3 + [P] * 2 + [Hh] * 2 + [P] * 2 + [A] * 3      # 88 .. 99: P and the flip back to it inside the 7-frame unit 91 .. 97
    seq = np.stack(seq)
    assert len(seq) == 100
    return seq


def _settle(settle):
    return settle if settle is not None else (0, 0)


def _flags(smalls, valid, settle, M, state=None):
    s = _settle(settle)
    return mref.flags(smalls, valid, CS, s[0], s[1], M, state)


def _conditions(smalls, valid=None, settles=SETTLES):
    """Conditions on the INPUT, by the restatement alone."""
    for settle in settles:
        by_m = {M: _flags(smalls, valid, settle, M) for M in MS}
        matches = [int(by_m[M][0].sum()) for M in MS]
        assert matches[0] > matches[1] > matches[2] >= matches[3], ("a larger memory matches fewer frames", settle, matches)
        assert not (by_m[1][2] == mref.RECALLED).any()
        ch, sim, kind, refs, state = by_m[4]
        rec = np.nonzero(kind == mref.RECALLED)[0]
        assert len(rec) >= 6, "the returns are recalled"
        for u in (7, 32):
            start = rec // u * u                                 # the first frame of the unit a recalled frame is in
            assert (refs[rec] < start).any() and (refs[rec] >= start).any(), "unit size %d: recalls of carried and of in-unit entries" % u
        # an eviction under the smallest memory: under M = 2 the two holds in between dropped D, and the return to it is matched again
        assert (by_m[2][2][35:37] == mref.MATCHED).any() and not (by_m[2][2][35:39] == mref.RECALLED).any()
        # the return to C over the fade: C is still remembered under M = 64 (under M = 4 the holds in between evicted it)
        rec64 = np.nonzero(by_m[64][2] == mref.RECALLED)[0]
        assert 42 < rec64[(rec64 >= 42) & (rec64 <= 70)].min() <= 68 and by_m[64][3][68] == by_m[64][3][14], "the return over the fade is recalled by the fade's end"
        assert by_m[4][2][68:71].max() >= mref.DEFERRED, "... and matched again under M = 4"
        assert kind[35] == mref.RECALLED and (kind[36:39] == mref.UNCHANGED).all() and refs[35] == refs[26], "the noisy hold returns to its own entry"
        if settle is not None:
            assert (kind == mref.DEFERRED).any() and (refs[kind == mref.DEFERRED] == mref.REF_DEFERRED).all()
            assert any((kind[b] == mref.DEFERRED) for b in (49, 56, 63, 64)), "a unit boundary inside a run of deferred frames"


def _matcher(capi, pages, settle=None, M=0, mask=None, t=None, anchor=True, scope=False):
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    if mask is not None or scope:
        m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    if mask is not None:
        m.set_frame_mask(mask)
    if t is not None:
        if mask is not None:
            m.set_direct_scope(capi.DIRECT_VALID)
        m.set_direct_similarity(t)
    if anchor:
        m.set_gate_reference("anchor")
    if settle is not None:
        m.set_gate_settle(*settle)
    if M:
        m.set_gate_memory(M)
        assert m.gate_memory() == M
    return m


class Want:
    """The definition over `seq` from the state "none" or a carried state: flags, similarities and refs from the restatement, verdicts
    and traces of the matched frames from match_frames on r (a plain call does not look at the gate), the others — unchanged,
    recalled and deferred alike — (-1, 0, 0, 0) or, `direct` (frame -> verdict), the look-up's."""

    def __init__(self, capi, r, seq, smalls, settle, M, valid=None, state=None, direct=None, yuv=None):
        self.changed, self.sims, self.kind, self.refs, self.state = _flags(smalls, valid, settle, M, state)
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


def _equal(want, got, refs, lo=0, hi=None, what=""):
    changed, sims, v = got
    hi = len(want.changed) if hi is None else hi
    assert len(changed) == hi - lo == len(refs), what
    assert np.array_equal(changed, want.changed[lo:hi]), (what, "flags", np.nonzero(changed != want.changed[lo:hi])[0][:8] + lo)
    assert sims.tobytes() == want.sims[lo:hi].tobytes(), (what, "similarities", np.nonzero(sims != want.sims[lo:hi])[0][:8] + lo)
    assert refs.dtype == np.int64 and np.array_equal(refs, want.refs[lo:hi]), (what, "refs", np.nonzero(refs != want.refs[lo:hi])[0][:8] + lo)
    assert v.tobytes() == want.v[lo:hi].tobytes(), (what, "verdicts", [i + lo for i in range(hi - lo) if v[i] != want.v[lo + i]][:8])


def _traces(want, m, what=""):
    for k, tr in enumerate(want.traces):
        assert m.last_candidates(k).tobytes() == tr, (what, "trace of pipeline frame %d" % k)


def _state(want, m, what=""):
    """The memory taps against the restatement's state."""
    E, a = want.state[0], want.state[1]
    ords, anchor = m.gate_memory_entries()
    assert ords.tolist() == [o for _, o in E] and anchor == a, (what, ords, anchor)
    for e in sorted({0, a, len(E) - 1}):
        assert np.array_equal(m.gate_memory_small(e), E[e][0]), (what, "entry", e)
    assert np.array_equal(m.gate_last_small(), E[a][0]), (what, "the last small image is the anchor's")


def _units(m, submit, n, unit):
    """Gated submit / collect in units of `unit`, max_in_flight at once, in order -> the concatenated result and refs (each ticket's
    refs are read behind its collect, with the later units still in flight)."""
    got, refs, pend = [], [], []

    def collect():
        got.append(m.collect_changed(pend.pop(0)))
        refs.append(m.last_gate_refs())

    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            collect()
        pend.append(submit(i, min(unit, n - i)))
    while pend:
        collect()
    return tuple(np.concatenate([g[j] for g in got]) for j in range(3)), np.concatenate(refs)


@pytest.fixture(scope="module")
def data(capi, synth):
    """-> pages, the stream, its small images (the shipped tap), the reference matcher r (PREVIOUS, no mask), a cache of definitions."""
    pages = synth.pages(4, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 8, W, H, threads=NCPU)
    r = _matcher(capi, pages, anchor=False)
    full = [r.reduce(pages[p], W, H) for p in (0, 3)]
    seq = _stream_frames(base, full)
    smalls = np.stack([r.small_image(f) for f in seq])
    assert smalls.shape[1:] == (259, 461, 3)
    _conditions(smalls)
    # the verdict of every frame, once: a Want picks the matched frames' (match_frames is per frame: a subset's verdicts are the
    # same bytes; the traces are taken per Want)
    wants = {}

    def want(settle, M):
        if (settle, M) not in wants:
            wants[(settle, M)] = Want(capi, r, seq, smalls, settle, M)
        return wants[(settle, M)]

    yield pages, seq, smalls, r, want
    r.close()


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("settle", SETTLES)
def test_synchronous_host_and_device(capi, data, settle, M):
    import torch
    pages, seq, smalls, _, want_of = data
    want = want_of(settle, M)
    m = _matcher(capi, pages, settle, M)
    with pytest.raises(capi.SlideoError) as e:
        m.last_gate_refs()
    assert e.value.code == 4, "no gated call since the setting"
    got = m.match_changed_frames(seq)
    _equal(want, got, m.last_gate_refs(), what="host, one call")
    _traces(want, m, "host, one call")
    _state(want, m, "host, one call")
    # several calls continue the ring, the previous frame, the count and the ordinals: cuts between a match and its recall, inside
    # the fade, a one-frame call
    m.gate_reset(None)
    cuts = (0, 8, 11, 12, 50, 64, 86, 100)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = m.match_changed_frames(seq[lo:hi])
        _equal(want, got, m.last_gate_refs(), lo, hi, "host call %d..%d" % (lo, hi))
    _state(want, m, "host calls")
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    got = m.match_changed_frames_dev(d.data_ptr(), len(seq), W, H)
    _equal(want, got, m.last_gate_refs(), what="device, one call")
    _traces(want, m, "device, one call")
    m.close()


UNIT_CASES = [(u, s, 4) for u in (1, 7, 32) for s in SETTLES] + [(7, None, 2), (7, (SETTLE, NEVER), 2), (32, None, 64), (7, (SETTLE, NEVER), 64), (7, (SETTLE, 4), 1)]


@pytest.mark.parametrize("unit,settle,M", UNIT_CASES)
def test_submit_collect_units(capi, data, unit, settle, M):
    import torch
    pages, seq, _, _, want_of = data
    want = want_of(settle, M)
    n, fb = len(seq), W * H * 3
    d = torch.from_numpy(seq).cuda()
    m = _matcher(capi, pages, settle, M)
    assert m.max_in_flight() > 1
    got, refs = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fb, c, W, H), n, unit)
    _equal(want, got, refs, what="units of %d" % unit)
    _traces(want, m, "units of %d" % unit)
    _state(want, m, "units of %d" % unit)
    m.close()


@pytest.mark.parametrize("settle", [None, (SETTLE, NEVER)])
def test_nv12_device_units(capi, data, settle):
    """4:2:0 frames stand for their BGR image: the small images of the conversion tap's output."""
    import torch
    pages, seq, _, r, _ = data
    L, fb = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(seq, L, fb)
    smalls = np.stack([r.small_image(r.yuv420_to_bgr(f, W, H, L)) for f in yuv])
    M = 4
    ch, _, kind, _, _ = _flags(smalls, None, settle, M)
    assert (kind == mref.RECALLED).sum() >= 6 and ch.sum() < _flags(smalls, None, settle, 1)[0].sum()
    want = Want(capi, r, yuv, smalls, settle, M, yuv=(W, H, L))
    d = torch.from_numpy(yuv).cuda()
    fs = yuv.shape[1]
    m = _matcher(capi, pages, settle, M)
    got, refs = _units(m, lambda i, c: m.submit_changed_yuv420_dev(d.data_ptr() + i * fs, c, W, H, L, fs), len(yuv), 7)
    _equal(want, got, refs, what="nv12 units of 7")
    _state(want, m, "nv12 units of 7")
    m.gate_reset(None)
    got = m.match_changed_frames_yuv420(yuv, W, H, L)
    _equal(want, got, m.last_gate_refs(), what="nv12 host")
    m.close()


@pytest.mark.parametrize("settle", SETTLES)
def test_m_1_is_anchor_byte_for_byte(capi, data, settle):
    """A memory of one entry against a matcher without a memory under the same settle, on every output, call by call."""
    pages, seq, _, _, _ = data
    a = _matcher(capi, pages, settle)
    s = _matcher(capi, pages, settle, 1)
    for lo, hi in ((0, 11), (11, 12), (12, 50), (50, 100)):
        ga, gs = a.match_changed_frames(seq[lo:hi]), s.match_changed_frames(seq[lo:hi])
        for x, y in zip(ga, gs):
            assert x.tobytes() == y.tobytes()
        assert [a.last_candidates(k).tobytes() for k in range(int(ga[0].sum()))] == [s.last_candidates(k).tobytes() for k in range(int(gs[0].sum()))]
        assert np.array_equal(a.gate_last_small(), s.gate_last_small())
    with pytest.raises(capi.SlideoError) as e:
        a.last_gate_refs()
    assert e.value.code == 4, "no memory: no refs"
    a.close()
    s.close()


def test_resets(capi, data):
    import torch
    pages, seq, smalls, r, _ = data
    settle, M = (SETTLE, NEVER), 4
    m = _matcher(capi, pages, settle, M)
    assert m.gate_memory_entries()[0].tolist() == [] and m.gate_memory_entries()[1] == -1
    # frames equal to S stand behind the reset's image; the stream then continues from ordinal 0
    for how in ("small", "frame"):
        if how == "small":
            m.gate_reset(smalls[0])
        else:
            m.gate_reset_from_frame(seq[0])
        ords, anchor = m.gate_memory_entries()
        assert ords.tolist() == [capi.GATE_REF_RESET] and anchor == 0 and np.array_equal(m.gate_memory_small(0), smalls[0])
        assert np.array_equal(m.gate_last_small(), smalls[0])
        want = Want(capi, r, seq[:21], smalls[:21], settle, M, state=mref.reset_state(smalls[0]))
        assert (want.refs[:5] == capi.GATE_REF_RESET).all() and (want.refs[10:13] == capi.GATE_REF_RESET).all(), "A, and the return to A"
        assert want.refs[6] == 6 and not want.changed[:5].any()
        if how == "small":
            got = m.match_changed_frames(seq[:21])
            _equal(want, got, m.last_gate_refs(), what="gate_reset(S)")
        else:
            d = torch.from_numpy(seq[:21]).cuda()
            got, refs = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), 21, 7)
            _equal(want, got, refs, what="gate_reset_from_frame, units of 7")
        _state(want, m, how)
    m.gate_reset(None)
    assert m.gate_memory_entries()[0].tolist() == []
    got = m.match_changed_frames(seq[:3])
    assert m.last_gate_refs().tolist() == [0, 0, 0] and got[0].tolist() == [1, 0, 0], "a reset to none leaves the next ordinal 0"
    m.close()


def test_mask_gate_scope_and_a_mask_change_between_calls(capi, oracle, data):
    pages, seq, _, _, _ = data
    settle, M = (SETTLE, NEVER), 4
    mask = np.full((H, W), 255, np.uint8)
    mask[HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = 0
    rng = np.random.default_rng(23)
    ins = seq.copy()
    for f in ins:
        f[INSET[0]:INSET[1], INSET[2]:INSET[3]] = rng.integers(0, 256, (INSET[1] - INSET[0], INSET[3] - INSET[2], 3), dtype=np.uint8)
    valid, nv = gref.validity_map(oracle, mask)
    rm = _matcher(capi, pages, anchor=False, mask=mask)          # (verdicts of the matched frames under the same detection mask)
    smalls = np.stack([rm.small_image(f) for f in ins])
    _conditions(smalls, valid, [settle])
    whole = _flags(smalls, None, settle, M)
    assert whole[0].sum() == 1 and (whole[2][1:] == mref.DEFERRED).all(), "unmasked, the inset keeps every frame away, none still, none recalled"
    want = Want(capi, rm, ins, smalls, settle, M, valid=valid)
    m = _matcher(capi, pages, settle, M, mask=mask)
    got = m.match_changed_frames(ins)
    _equal(want, got, m.last_gate_refs(), what="mask, host")
    _traces(want, m, "mask, host")
    _state(want, m, "mask: the memory's images are whole")
    import torch
    d = torch.from_numpy(ins).cuda()
    m.gate_reset(None)
    got, refs = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(ins), 7)
    _equal(want, got, refs, what="mask, units of 7")
    m.close()
    # a mask set between two calls keeps the gate state: the second call compares the remembered WHOLE images under the new map
    cut = 27
    plain = seq[:cut]
    r = data[3]
    psm = np.stack([r.small_image(f) for f in plain])
    w0 = Want(capi, r, plain, psm, None, M)
    w1 = Want(capi, rm, ins[cut:], smalls[cut:], None, M, valid=valid, state=w0.state)
    assert (w1.kind == mref.RECALLED).any() and (w1.refs[w1.kind == mref.RECALLED] < cut).any(), "entries remembered before the mask are recalled under it"
    assert not np.array_equal(w1.changed, _flags(smalls[cut:], None, None, M, w0.state)[0]), "the new map matters"
    m = _matcher(capi, pages, None, M, scope=True)
    got = m.match_changed_frames(plain)
    _equal(w0, got, m.last_gate_refs(), what="before the mask")
    m.set_frame_mask(mask)
    got = m.match_changed_frames(ins[cut:])
    _equal(w1, got, m.last_gate_refs(), what="behind the mask change")
    _state(w1, m, "behind the mask change")
    m.close()
    rm.close()


def test_direct_similarity_sees_matched_frames_only(capi, data):
    pages, seq, smalls, r, want_of = data
    settle, M = None, 4
    base = want_of(settle, M)
    ssd = r.page_small_ssd(smalls).astype(np.int64)              # the shipped tap, on the reference matcher
    best = ssd.min(axis=1)
    page = ssd.argmin(axis=1)                                    # (the lowest page with the smallest SSD)
    sims = np.array([gref.similarity(int(b), 259 * 461) for b in best], np.float32)
    full = np.zeros(len(seq), bool)
    full[27:31] = True
    full[71:77] = True
    full[85:88] = True
    lo, hi = float(sims[~full].max()), float(sims[full].min())
    assert lo < hi, "the full-screen slide frames are closer to their page than any other frame to any"
    t = float(np.float32((lo + hi) / 2))
    direct = {int(i): (int(page[i]), sims[i], 0, 0) for i in np.nonzero(base.changed)[0] if sims[i] >= np.float32(t)}
    assert sorted(direct) == [27, 71] and [direct[27][0], direct[71][0]] == [0, 3]
    assert base.kind[85] == mref.RECALLED and sims[85] >= np.float32(t), "the return to G is recalled: the look-up never sees it"
    want = Want(capi, r, seq, smalls, settle, M, direct=direct)
    assert np.array_equal(want.changed, base.changed) and len(want.pipe) == int(base.changed.sum()) - 2
    m = _matcher(capi, pages, settle, M, t=t)
    got = m.match_changed_frames(seq)
    _equal(want, got, m.last_gate_refs(), what="direct, host")
    _traces(want, m, "direct, host")
    import torch
    d = torch.from_numpy(seq).cuda()
    m.gate_reset(None)
    got, refs = _units(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * W * H * 3, c, W, H), len(seq), 32)
    _equal(want, got, refs, what="direct, units of 32")
    _state(want, m, "direct")
    m.close()


def test_setter_rules_and_the_record_calls(capi, data):
    import torch
    pages, seq, smalls, _, _ = data
    m = _matcher(capi, pages, anchor=False)
    assert m.gate_memory() == 0
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_memory(4)
    assert e.value.code == 5 and "SLIDEO_GATE_ANCHOR" in str(e.value) and m.gate_memory() == 0, "a memory under PREVIOUS"
    m.set_gate_memory(0)                                         # off is accepted under PREVIOUS
    m.set_gate_reference("anchor")
    for bad in (-1, 65):
        assert capi.lib().slideo_matcher_set_gate_memory(m._h, bad) == 1 and m.gate_memory() == 0
    m.set_gate_memory(4)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_reference("previous")
    assert e.value.code == 5 and m.gate_reference() == "anchor" and m.gate_memory() == 4, "PREVIOUS while a memory is on"
    for bad in (-1, 65):
        assert capi.lib().slideo_matcher_set_gate_memory(m._h, bad) == 1 and m.gate_memory() == 4, "the value before stays"
    d = torch.from_numpy(seq[:4]).cuda()
    t = m.submit_changed_dev(d.data_ptr(), 4, W, H)
    with pytest.raises(capi.SlideoError) as e:
        m.set_gate_memory(5)
    assert e.value.code == 4 and m.gate_memory() == 4, "the setter needs an idle matcher"
    with pytest.raises(capi.SlideoError) as e:
        m.gate_memory_entries()
    assert e.value.code == 4, "the taps too"
    m.collect_changed(t)
    assert m.last_gate_refs().tolist() == [0, 0, 0, 0]
    assert np.array_equal(m.gate_last_small(), smalls[0])
    # the record calls refuse while a memory is on, by name, and the state stays
    n64 = __import__("ctypes").c_int64(-7)
    assert capi.lib().slideo_matcher_gate_state_bytes(m._h, __import__("ctypes").byref(n64)) == 5 and n64.value == -7
    for call in (m.gate_state_export, lambda: m.gate_state_import(b"\0" * 32)):
        with pytest.raises(capi.SlideoError) as e:
            call()
        assert e.value.code == 5 and "gate memory" in str(e.value)
    assert m.gate_memory_entries()[0].tolist() == [0]
    for M in (4, 4, 0):                                          # setting it resets the gate state, also to the value in force
        m.gate_reset(smalls[0])
        m.set_gate_memory(M)
        with pytest.raises(capi.SlideoError) as e:
            m.gate_last_small()
        assert e.value.code == 4
    with pytest.raises(capi.SlideoError) as e:
        m.last_gate_refs()
    assert e.value.code == 4, "M == 0"
    m.gate_reset(smalls[0])                                      # ... and with M = 0 the record works again
    rec = m.gate_state_export()
    assert len(rec) == 32 + smalls[0].size
    m.gate_state_import(rec)
    assert np.array_equal(m.gate_last_small(), smalls[0])
    m.set_gate_reference("previous")                             # the memory is off: accepted
    m.close()


def test_groups(capi, data):
    pages, seq, _, _, want_of = data
    settle, M = (SETTLE, NEVER), 4
    want = want_of(settle, M)
    g = capi.Group(small_cfg(capi), devices=[0])
    g.add_pages(list(pages))
    g.finalize()
    g.set_gate_reference("anchor")
    g.set_gate_settle(*settle)
    g.set_gate_memory(M)
    assert g.gate_memory() == M
    got = g.match_changed_frames(seq[:50])
    _equal(want, got, g.last_gate_refs(), 0, 50, "group of one")
    got = g.match_changed_frames(seq[50:])
    _equal(want, got, g.last_gate_refs(), 50, 100, "group of one, second call")
    assert np.array_equal(g.gate_last_small(), want.state[0][want.state[1]][0])
    with pytest.raises(capi.SlideoError) as e:
        g.gate_state_export()
    assert e.value.code == 5
    g.close()
    g2 = capi.Group(small_cfg(capi), devices=[0, 0])
    g2.set_gate_order("chain")
    g2.set_gate_reference("anchor")
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_memory(M)
    assert e.value.code == 5 and "members" in str(e.value)
    assert [g2.member(i).gate_memory() for i in range(2)] == [0, 0], "no member is changed"
    g2.set_gate_memory(0)                                        # off: always accepted
    with pytest.raises(capi.SlideoError) as e:
        g2.set_gate_memory(65)
    assert e.value.code == 1
    with pytest.raises(capi.SlideoError) as e:
        g2.last_gate_refs()
    assert e.value.code == 4
    g2.close()
    # the mirror: the refusal surfaces when the group is built
    from slideo_amd import matching
    with pytest.raises(capi.SlideoError) as e:
        matching.HipImageVideoMatcher(cfg=small_cfg(capi), devices=[0], gate_memory=4).create_video_matcher(
            [], matching.ProgressReporter(lambda *a: None))
    assert e.value.code == 5, "a memory under the PREVIOUS default"
