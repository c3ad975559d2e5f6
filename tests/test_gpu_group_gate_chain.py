"""The group gate order CHAIN and the gate state record (include/slideo_amd.h "Group gate order", "Gate state record") on the GPU.

The single matcher is the bit-for-bit twin: a group under CHAIN returns, for the same sequence of resets and gated calls, the twin's
flags, similarities (compared as uint32), verdict records, traces, gate_last_small and exported record — for 2, 3 and 5 members on
one device, for the stream as one call, as calls of 1, 7 and 16 frames and after a call with fewer frames than members.  The numpy
restatements (tests/gate_anchor_ref.py, tests/gate_settle_ref.py, tests/gate_mask_ref.py) over small images from the shipped tap are
the check on the twin, and `_conditions` asserts on them, before anything is compared, that the stream's shard boundaries do what
they were chosen for: one is crossed with a deferral count > 0, one shard flags no frame, one shard's first frame is matched.

The stream (`stream_frames`, 48 frames of 640x360): a hold (0 .. 3), a hard cut into a 16-step fade (4 .. 24: three frames of its
first picture, 15 steps, three frames of its last), a full-screen slide (25 .. 30), a hold (31 .. 36), a hold under +-3 noise
(37 .. 42) and a last hold (43 .. 47).  With 2, 3 and 5 members the shards of the one-call case begin at 24; 16, 32; 10, 20, 30, 39:
10, 16 and 20 lie inside the fade."""
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
N = 48
MEMBERS = (2, 3, 5)
# (gate reference, settle) of the cases
PREVIOUS, ANCHOR, SETTLE_NEVER, SETTLE_3 = ("previous", None), ("anchor", None), ("anchor", (SETTLE, NEVER)), ("anchor", (SETTLE, 3))


def stream_frames(base, full):
    """base: eight synthetic frames; full: a full-screen slide frame (a page reduced to the frame size)."""
    a64, b64 = base[1].astype(np.float64), base[2].astype(np.float64)
    seq = [base[0]] * 4
    seq += [base[1]] * 3 + [np.rint(a64 + (b64 - a64) * j / 16).astype(np.uint8) for j in range(1, 16)] + [base[2]] * 3      # 4 .. 24
    seq += [full] * 6                                            # 25 .. 30
    seq += [base[4]] * 6                                         # 31 .. 36
    noise = np.random.default_rng(19)
    seq += [np.clip(base[5].astype(np.int16) + noise.integers(-3, 4, base[5].shape), 0, 255).astype(np.uint8) for _ in range(6)]      # 37 .. 42
    seq += [base[6]] * 5                                         # 43 .. 47
    seq = np.stack(seq)
    assert len(seq) == N
    return seq


def shard_bounds(n, members):
    """The group's contiguous shards of a call of n frames (slideo_amd/distributed.py shard_range) -> [(lo, hi)] of the non-empty ones."""
    base, rem = divmod(n, members)
    out, lo = [], 0
    for r in range(members):
        hi = lo + base + (1 if r < rem else 0)
        if hi > lo:
            out.append((lo, hi))
        lo = hi
    return out


def call_cuts(members):
    """The call patterns of the matrix -> {name: the calls' bounds}."""
    few = members - 1                                            # a call with fewer frames than members, then the rest
    return {"one call": [0, N], "calls of 1": list(range(N + 1)), "calls of 7": list(range(0, N, 7)) + [N],
            "calls of 16": [0, 16, 32, N], "fewer frames than members": [0, few, N]}


def all_shards(members_list=MEMBERS):
    """Every shard [lo, hi) of the stream that some case of the matrix gives to a member of its own."""
    out = set()
    for members in members_list:
        for cuts in call_cuts(members).values():
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                out.update((lo + a, lo + b) for a, b in shard_bounds(hi - lo, members))
    return sorted(out)


def restated(smalls, case, valid=None, state=None):
    """-> (changed, similarity, d in front of each frame or None, the state behind) by the numpy restatement of the case's rule."""
    ref, settle = case
    if ref == "previous":
        n = int(valid.sum()) if valid is not None else smalls.shape[1] * smalls.shape[2]
        v = valid if valid is not None else np.ones(smalls.shape[1:3], bool)
        ch, sim = np.zeros(len(smalls), bool), np.zeros(len(smalls), np.float32)
        prev = state
        for i, s in enumerate(smalls):
            sim[i] = np.float32(0.0) if prev is None else gref.similarity(gref.masked_ssd(prev, s, v), n)
            ch[i] = prev is None or sim[i] < np.float32(CS)
            prev = s
        return ch, sim, None, prev
    if settle is None:
        ch, sim, _, last = aref.flags(smalls, valid, CS)
        return ch, sim, None, last
    ch, sim, _, d, st = sref.flags(smalls, valid, CS, settle[0], settle[1], state)
    return ch, sim, d, st


def _conditions(smalls, case):
    """Conditions on the INPUT, by the restatement alone: what the shard boundaries of the matrix cross."""
    ch, _, d, _ = restated(smalls, case)
    shards = all_shards()
    assert any(not ch[lo:hi].any() for lo, hi in shards), "some shard flags no frame: the anchor passes through a member untouched"
    assert any(ch[lo] for lo, _ in shards if lo > 0), "some shard's first frame is matched"
    if d is not None:
        assert any(d[lo] > 0 for lo, _ in shards if lo > 0), "some shard boundary is crossed with d > 0: a deferred run spans two members"
        one = [lo for m in MEMBERS for lo, _ in shard_bounds(N, m) if lo > 0]
        if case[1][1] == NEVER:
            assert any(d[lo] > 1 for lo in one), "in the one-call case too, deep inside the fade"
    return ch


def _setup(obj, capi, case, mask=None, t=None, order=None):
    ref, settle = case
    if mask is not None:
        obj.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        obj.set_frame_mask(mask)
    if t is not None:
        if mask is not None:
            obj.set_direct_scope(capi.DIRECT_VALID)
        obj.set_direct_similarity(t)
    if order is not None:
        obj.set_gate_order(order)
    obj.set_gate_reference(ref)
    if settle is not None:
        obj.set_gate_settle(*settle)
    return obj


def _matcher(capi, pages, case=PREVIOUS, **kw):
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(list(pages))
    m.finalize()
    return _setup(m, capi, case, **kw)


def _group(capi, pages, members, case=PREVIOUS, order="chain", **kw):
    g = capi.Group(small_cfg(capi), devices=[0] * members)
    g.add_pages(list(pages))
    g.finalize()
    return _setup(g, capi, case, order=order, **kw)


FIELDS = ("flags", "similarities as uint32", "verdict records", "traces", "gate_last_small", "the exported record")


def _direct(v):
    return (v["page_idx"] >= 0) & (v["inliers"] == 0)


def _run(obj, seq, cuts, reset=None, call=None):
    """gate_reset(reset), then the stream as the calls `cuts` -> per call everything the definition names, as bytes."""
    call = call or (lambda o, lo, hi: o.match_changed_frames(seq[lo:hi]))
    obj.gate_reset(reset)
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ch, sims, v = call(obj, lo, hi)
        pipe = int((ch & ~_direct(v)).sum())                     # the frames that went through the pipeline: changed and not direct
        out.append((ch.tobytes(), np.ascontiguousarray(sims).view(np.uint32).tobytes(), v.tobytes(),
                    [obj.last_candidates(k).tobytes() for k in range(pipe)], obj.gate_last_small().tobytes(), obj.gate_state_export()))
    return out


def _same(want, got, what):
    assert len(want) == len(got), what
    for c, (a, b) in enumerate(zip(want, got)):
        for name, x, y in zip(FIELDS, a, b):
            assert x == y, (what, "call %d" % c, name)


def _flat(runs, capi):
    ch = np.concatenate([np.frombuffer(r[0], np.uint8) for r in runs]).astype(bool)
    sims = np.concatenate([np.frombuffer(r[1], np.float32) for r in runs])
    v = np.concatenate([np.frombuffer(r[2], capi.VERDICT_DTYPE) for r in runs])
    return ch, sims, v


def parse_record(rec):
    """-> (has, gate reference, settle, sw, sh, d, anchor, previous image) of a record, by the layout the public header states."""
    w = np.frombuffer(rec[:32], "<u4")
    assert w[0] == 0x54534753 and w[1] == 1
    has, ref, settle, sw, sh, d = (int(x) for x in w[2:8])
    sb = sw * sh * 3
    assert len(rec) == 32 + (sb * (2 if settle else 1) if has else 0)
    img = lambda k: np.frombuffer(rec[32 + k * sb:32 + (k + 1) * sb], np.uint8).reshape(sh, sw, 3)
    return has, ref, settle, sw, sh, d, (img(0) if has else None), (img(1) if has and settle else None)


class Twin:
    """The single matcher of one case and, per call pattern, what it returns (computed once, shared, never changed)."""

    def __init__(self, capi, pages, seq, smalls, case, **kw):
        self.capi, self.seq, self.case, self.kw = capi, seq, case, kw
        self.m = _matcher(capi, pages, case, **kw)
        self.runs = {}
        self.restated = restated(smalls, case, kw.get("valid"))

    def run(self, cuts, reset=None, seq=None, call=None):
        key = (tuple(cuts), None if reset is None else reset.tobytes())
        if key not in self.runs:
            self.runs[key] = _run(self.m, self.seq if seq is None else seq, cuts, reset, call)
            if reset is None and cuts[0] == 0:                   # the check on the twin: flags and similarities of the restatement
                ch, sims, _ = _flat(self.runs[key], self.capi)
                assert np.array_equal(ch, self.restated[0][:cuts[-1]]), "the twin's flags are the restatement's"
                assert sims.tobytes() == self.restated[1][:cuts[-1]].tobytes(), "the twin's similarities are the restatement's"
        return self.runs[key]


@pytest.fixture(scope="module")
def data(capi, synth):
    pages = synth.pages(6, 800, 450, threads=NCPU)
    base, _, _ = synth.frames(pages, 8, W, H, threads=NCPU)
    r = _matcher(capi, pages)
    full = r.reduce(pages[3], W, H)
    seq = stream_frames(base, full)
    smalls = np.stack([r.small_image(f) for f in seq])
    twins = {}

    def twin(case):
        if case not in twins:
            _conditions(smalls, case)
            twins[case] = Twin(capi, pages, seq, smalls, case)
        return twins[case]

    yield pages, seq, smalls, r, twin
    for t in twins.values():
        t.m.close()
    r.close()


def _matrix(capi, data, case, members):
    pages, seq, smalls, _, twin = data
    tw = twin(case)
    g = _group(capi, pages, members, case)
    assert g.gate_order() == "chain" and g.gate_reference() == case[0]
    for name, cuts in call_cuts(members).items():
        _same(tw.run(cuts), _run(g, seq, cuts), "%s, %d members, %s" % (case, members, name))
    g.close()


# ---- 1: ANCHOR under CHAIN ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
def test_anchor_under_chain(capi, data, members):
    _matrix(capi, data, ANCHOR, members)


# ---- 2: the settle under CHAIN --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
@pytest.mark.parametrize("case", [SETTLE_NEVER, SETTLE_3], ids=["never", "cap3"])
def test_settle_under_chain(capi, data, case, members):
    _matrix(capi, data, case, members)


@pytest.mark.parametrize("case", [SETTLE_NEVER, SETTLE_3], ids=["never", "cap3"])
def test_the_twins_state_at_the_shard_boundaries(capi, data, case):
    """The single matcher's exported state at every shard boundary of the one-call cases: anchor, previous frame and d of the restatement."""
    pages, seq, smalls, _, twin = data
    ch, _, d, _ = twin(case).restated
    m = _matcher(capi, pages, case)
    bounds = sorted({lo for mem in MEMBERS for lo, _ in shard_bounds(N, mem) if lo > 0})
    assert bounds == [10, 16, 20, 24, 30, 32, 39]
    seen_d = []
    for b in bounds:
        m.gate_reset(None)
        m.match_changed_frames(seq[:b])
        has, ref, settle, sw, sh, rd, anchor, prev = parse_record(m.gate_state_export())
        assert (has, ref, settle, sw, sh) == (1, capi.GATE_ANCHOR, 1, 461, 259)
        assert rd == d[b], "d in front of frame %d" % b
        assert np.array_equal(anchor, smalls[np.nonzero(ch[:b])[0].max()]) and np.array_equal(prev, smalls[b - 1])
        seen_d.append(rd)
    assert max(seen_d) > 0
    m.close()


# ---- 3: PREVIOUS: CHAIN = HALO = the single matcher ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
def test_previous_chain_equals_halo_equals_single(capi, data, members):
    pages, seq, smalls, _, twin = data
    tw = twin(PREVIOUS)
    for order in ("chain", "halo"):
        g = _group(capi, pages, members, PREVIOUS, order=order)
        assert g.gate_order() == order
        for name, cuts in call_cuts(members).items():
            _same(tw.run(cuts), _run(g, seq, cuts), "PREVIOUS, %s, %d members, %s" % (order, members, name))
        g.close()


# ---- 4: one case each under CHAIN + ANCHOR + settle -----------------------------------------------------------------------------------------
def test_nv12(capi, data):
    pages, seq, _, r, _ = data
    L, fb = capi.yuv420_layout("nv12", W, H)
    yuv = yref.frames_to_yuv(seq, L, fb)
    smalls = np.stack([r.small_image(r.yuv420_to_bgr(f, W, H, L)) for f in yuv])
    _conditions(smalls, SETTLE_NEVER)
    tw = Twin(capi, pages, yuv, smalls, SETTLE_NEVER)
    call = lambda o, lo, hi: o.match_changed_frames_yuv420(yuv[lo:hi], W, H, L)
    g = _group(capi, pages, 3, SETTLE_NEVER)
    for cuts in ([0, N], [0, 7, 14, 30, N]):
        _same(tw.run(cuts, call=call), _run(g, yuv, cuts, call=call), "nv12, %s" % cuts)
    g.close()
    tw.m.close()


def test_frame_mask_under_the_gate_scope(capi, oracle, data):
    pages, seq, _, _, _ = data
    mask = np.full((H, W), 255, np.uint8)
    mask[190:350, 390:630] = 0
    rng = np.random.default_rng(23)
    ins = seq.copy()
    for f in ins:                                                # an inset renewed on every frame, inside the masked region
        f[191:349, 391:629] = rng.integers(0, 256, (158, 238, 3), dtype=np.uint8)
    valid, _ = gref.validity_map(oracle, mask)
    rm = _matcher(capi, pages, mask=mask)
    smalls = np.stack([rm.small_image(f) for f in ins])
    rm.close()
    whole = sref.flags(smalls, None, CS, SETTLE, NEVER)
    assert whole[0].sum() == 1, "unmasked, the inset keeps every frame away and none still"
    tw = Twin(capi, pages, ins, smalls, SETTLE_NEVER, mask=mask)
    tw.restated = restated(smalls, SETTLE_NEVER, valid)
    assert tw.restated[0].sum() > 3
    g = _group(capi, pages, 3, SETTLE_NEVER, mask=mask)
    for cuts in ([0, N], [0, 7, 14, 30, N]):
        _same(tw.run(cuts), _run(g, ins, cuts), "mask under the gate scope, %s" % cuts)
    g.close()
    tw.m.close()


def test_direct_look_up(capi, data):
    pages, seq, smalls, r, twin = data
    base = twin(SETTLE_NEVER).restated[0]
    ssd = r.page_small_ssd(smalls).astype(np.int64)              # the shipped tap, on the reference matcher
    sims = np.array([gref.similarity(int(b), 259 * 461) for b in ssd.min(axis=1)], np.float32)
    full = np.zeros(N, bool)
    full[25:31] = True
    lo, hi = float(sims[~full].max()), float(sims[full].min())
    assert lo < hi, "the full-screen slide frames are closer to their page than any other frame to any"
    t = float(np.float32((lo + hi) / 2))
    tw = Twin(capi, pages, seq, smalls, SETTLE_NEVER, t=t)
    g = _group(capi, pages, 3, SETTLE_NEVER, t=t)
    for cuts in ([0, N], [0, 7, 14, 30, N]):
        want = tw.run(cuts)
        ch, _, v = _flat(want, capi)
        d = _direct(v)
        assert d.any() and (ch & ~d).any() and np.array_equal(np.nonzero(d)[0], np.nonzero(base & full)[0]), "some changed frames are direct, the others go through the pipeline"
        assert (v["page_idx"][d] == 3).all()
        _same(want, _run(g, seq, cuts), "direct look-up, %s" % cuts)     # (the traces are indexed by the group's match_lo)
    g.close()
    tw.m.close()


def test_page_set(capi, data):
    pages, seq, smalls, _, _ = data
    tw = Twin(capi, pages, seq, smalls, SETTLE_NEVER)
    g = _group(capi, pages, 3, SETTLE_NEVER)
    sets = [o.create_page_set([0, 2, 3]) for o in (tw.m, g)]
    assert sets[0] == sets[1]
    tw.m.use_page_set(sets[0])
    g.use_page_set(sets[1])
    want = tw.run([0, N])
    _, _, v = _flat(want, capi)
    assert set(v["page_idx"][v["page_idx"] >= 0].tolist()) <= {0, 2, 3}
    _same(want, _run(g, seq, [0, N]), "page set")
    g.close()
    tw.m.close()


def test_group_reset_with_a_small_image_between_calls(capi, data):
    pages, seq, smalls, _, twin = data
    tw = twin(SETTLE_NEVER)
    g = _group(capi, pages, 3, SETTLE_NEVER)
    _same(tw.run([0, 14]), _run(g, seq, [0, 14]), "the first call")
    # frame 15 against anchor = previous = frame 9, d = 0: the reset's image decides, not what the first call left
    want = tw.run([15, 30, N], reset=smalls[9])
    _same(want, _run(g, seq, [15, 30, N], reset=smalls[9]), "behind gate_reset(small image)")
    g.gate_reset(smalls[9])
    has, _, settle, _, _, d, anchor, prev = parse_record(g.gate_state_export())
    assert (has, settle, d) == (1, 1, 0) and np.array_equal(anchor, smalls[9]) and np.array_equal(prev, smalls[9])
    tw.m.gate_reset(smalls[9])
    assert g.gate_state_export() == tw.m.gate_state_export()
    g.gate_reset(None)
    tw.m.gate_reset(None)
    assert parse_record(g.gate_state_export())[0] == 0 and g.gate_state_export() == tw.m.gate_state_export()
    g.close()


# ---- 5: the record on single matchers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [PREVIOUS, ANCHOR, SETTLE_NEVER, SETTLE_3], ids=["previous", "anchor", "never", "cap3"])
def test_a_stream_continues_on_another_matcher(capi, data, case):
    pages, seq, smalls, _, twin = data
    tw = twin(case)
    whole = tw.run([0, N])[0]
    d = tw.restated[2]
    for cut in (28, 14):                                         # inside the slide's hold; inside the fade
        if d is not None:
            assert (d[cut] > 0) == (cut == 14), "the fade is cut with d > 0"
        a, b = _matcher(capi, pages, case), _matcher(capi, pages, case)
        first = _run(a, seq, [0, cut])
        rec = a.gate_state_export()
        b.gate_state_import(rec)
        assert b.gate_state_export() == rec and b.gate_last_small().tobytes() == a.gate_last_small().tobytes()
        ch, sims, v = b.match_changed_frames(seq[cut:])
        assert first[0][0] + ch.tobytes() == whole[0], ("flags", cut)
        assert first[0][1] + sims.view(np.uint32).tobytes() == whole[1], ("similarities", cut)
        assert first[0][2] + v.tobytes() == whole[2], ("verdicts", cut)
        assert b.gate_last_small().tobytes() == whole[4] and b.gate_state_export() == whole[5]
        a.close()
        b.close()
    if case == SETTLE_NEVER:
        # what the record is for: the anchor's small image alone does not continue this stream
        a, b = _matcher(capi, pages, case), _matcher(capi, pages, case)
        a.match_changed_frames(seq[:14])
        b.gate_reset(a.gate_last_small())
        assert b.gate_state_export() != a.gate_state_export()
        a.close()
        b.close()


def test_import_refusals_leave_the_state(capi, data):
    import torch
    pages, seq, smalls, _, twin = data
    tw = twin(SETTLE_NEVER)
    whole = tw.run([0, N])[0]
    a, b = _matcher(capi, pages, SETTLE_NEVER), _matcher(capi, pages, SETTLE_NEVER)
    a.match_changed_frames(seq[:14])
    rec = a.gate_state_export()
    b.gate_state_import(rec)
    u32 = lambda v: np.array([v], "<u4").tobytes()
    big = u32(0x54534753) + u32(1) + u32(1) + u32(1) + u32(1) + u32(500) + u32(300) + u32(0)
    assert 500 * 300 > b.cfg.small_area
    other_ref = _matcher(capi, pages, PREVIOUS)
    other_ref.match_changed_frames(seq[:3])
    no_settle = _matcher(capi, pages, ANCHOR)
    no_settle.match_changed_frames(seq[:3])
    bad = {"one byte short": rec[:-1], "one byte long": rec + b"\0", "a header cut short": rec[:31], "empty": b"",
           "a bad magic": b"X" + rec[1:], "a bad version": rec[:4] + u32(2) + rec[8:],
           "another gate reference": other_ref.gate_state_export(), "the settle off": no_settle.gate_state_export(),
           "a small image beyond small_area": big + bytes(500 * 300 * 3 * 2), "sw 0": rec[:20] + u32(0) + rec[24:]}
    for what, r in bad.items():
        with pytest.raises(capi.SlideoError) as e:
            b.gate_state_import(r)
        assert e.value.code == 1 and "gate state record" in str(e.value), what
        assert b.gate_state_export() == rec, what
    # ... and into a matcher under PREVIOUS the settle's record is refused too
    with pytest.raises(capi.SlideoError) as e:
        other_ref.gate_state_import(rec)
    assert e.value.code == 1
    # units in flight: SLIDEO_ERR_STATE, on import, export and the size
    d = torch.from_numpy(seq[14:18]).cuda()
    t = b.submit_changed_dev(d.data_ptr(), 4, W, H)
    for f in (lambda: b.gate_state_import(rec), lambda: b.gate_state_export()):
        with pytest.raises(capi.SlideoError) as e:
            f()
        assert e.value.code == 4
    ch, sims, v = b.collect_changed(t)
    ch2, sims2, v2 = b.match_changed_frames(seq[18:])
    assert ch.tobytes() + ch2.tobytes() == whole[0][14:], "the refused calls changed nothing"
    assert v.tobytes() + v2.tobytes() == whole[2][14 * v.itemsize:]
    assert b.gate_state_export() == whole[5]
    # a record of "none" imports as gate_reset(None)
    a.gate_reset(None)
    none = a.gate_state_export()
    assert len(none) == 32 and parse_record(none)[0] == 0
    b.gate_state_import(none)
    with pytest.raises(capi.SlideoError) as e:
        b.gate_last_small()
    assert e.value.code == 4
    assert b.match_changed_frames(seq[:2])[0].tolist() == [True, False]
    for m in (a, b, other_ref, no_settle):
        m.close()


# ---- 6: the setter's rules on a two-member group -------------------------------------------------------------------------------------------
def test_setter_rules(capi, data):
    import torch
    pages, seq, smalls, _, twin = data
    g = capi.Group(small_cfg(capi), devices=[0, 0])
    g.add_pages(list(pages))
    g.finalize()
    assert g.gate_order() == "halo"
    for f in (lambda: g.set_gate_reference("anchor"), lambda: g.set_gate_settle(SETTLE, NEVER)):
        with pytest.raises(capi.SlideoError) as e:
            f()
        assert e.value.code == 5 and "one member" in str(e.value), "the default still refuses"
    g.set_gate_order("chain")
    g.set_gate_reference("anchor")
    g.set_gate_settle(SETTLE, 3)
    assert [g.member(i).gate_reference() for i in range(2)] == ["anchor", "anchor"]
    assert [g.member(i).gate_settle() for i in range(2)] == [(float(np.float32(SETTLE)), 3)] * 2
    with pytest.raises(capi.SlideoError) as e:
        g.set_gate_order("halo")
    assert e.value.code == 5 and g.gate_order() == "chain", "HALO while a settle is on"
    g.set_gate_settle(0, 0)
    with pytest.raises(capi.SlideoError) as e:
        g.set_gate_order("halo")
    assert e.value.code == 5 and g.gate_order() == "chain", "HALO under ANCHOR"
    for bad in (2, 7, 0xFFFFFFFF):
        with pytest.raises(capi.SlideoError) as e:
            g.set_gate_order(bad)
        assert e.value.code == 1 and g.gate_order() == "chain"
    g.set_gate_settle(SETTLE, NEVER)
    # a successful set resets the group's state, also to the value in force
    g.match_changed_frames(seq[:3])
    assert parse_record(g.gate_state_export())[0] == 1
    g.set_gate_order("chain")
    assert parse_record(g.gate_state_export())[0] == 0
    # a member busy: SLIDEO_ERR_STATE, the value stays
    d = torch.from_numpy(seq[:2]).cuda()
    m1 = g.member(1)
    t = m1.submit_changed_dev(d.data_ptr(), 2, W, H)
    for f in (lambda: g.set_gate_order("chain"), lambda: g.gate_state_export(), lambda: g.gate_state_import(b"")):
        with pytest.raises(capi.SlideoError) as e:
            f()
        assert e.value.code in (1, 4)
    with pytest.raises(capi.SlideoError) as e:
        g.set_gate_order("chain")
    assert e.value.code == 4
    m1.collect_changed(t)
    # a gated call that fails validation leaves the group's state and record as they were
    g.gate_reset(None)
    want = twin(SETTLE_NEVER).run([0, 14, N])
    ch, sims, v = g.match_changed_frames(seq[:14])
    rec = g.gate_state_export()
    assert rec == want[0][5]
    with pytest.raises(capi.SlideoError) as e:
        g.match_changed_frames(np.zeros((3, 180, 320, 3), np.uint8))
    assert e.value.code == 4, "another frame size without a reset"
    assert g.gate_state_export() == rec
    ch2, sims2, v2 = g.match_changed_frames(seq[14:])
    assert ch2.tobytes() == want[1][0] and v2.tobytes() == want[1][2] and g.gate_state_export() == want[1][5]
    # the group's import: a single matcher's record continues on the group, a refused one leaves it
    a = _matcher(capi, pages, SETTLE_NEVER)
    a.match_changed_frames(seq[:14])
    g.gate_reset(smalls[0])
    before = g.gate_state_export()
    with pytest.raises(capi.SlideoError) as e:
        g.gate_state_import(rec[:-1])
    assert e.value.code == 1 and g.gate_state_export() == before
    g.gate_state_import(a.gate_state_export())
    ch3, _, v3 = g.match_changed_frames(seq[14:])
    assert ch3.tobytes() == want[1][0] and v3.tobytes() == want[1][2] and g.gate_state_export() == want[1][5]
    a.close()
    # going back: settle off, PREVIOUS, then HALO
    g.set_gate_settle(0, 0)
    g.set_gate_reference("previous")
    g.set_gate_order("halo")
    assert g.gate_order() == "halo"
    g.close()
    one = capi.Group(small_cfg(capi), devices=[0])               # a group of one takes every combination
    one.set_gate_reference("anchor")
    one.set_gate_order("chain")
    one.set_gate_order("halo")
    one.close()


# ---- 7: the mirror ------------------------------------------------------------------------------------------------------------------------------
def test_the_mirror_runs_anchor_and_settle_on_two_members(capi, data, tmp_path):
    from slideo_amd import matching
    pages, seq, _, _, _ = data

    from PIL import Image

    class Page:
        def __init__(self, path, nr):
            self.path, self.page_nr = path, nr

        def get_path(self):
            return self.path

        def __eq__(self, o):
            return isinstance(o, Page) and o.page_nr == self.page_nr

    objs = []
    for i, p in enumerate(pages):
        path = str(tmp_path / ("p-%d.png" % (i + 1)))
        Image.fromarray(np.ascontiguousarray(p[:, :, ::-1])).save(path)
        objs.append(Page(path, i + 1))
    video = str(tmp_path / "v.slvf")
    matching.RawVideo.write(video, seq, fps=0.2)                 # one sample per frame
    out = {}
    for devices in ([0], [0, 0]):
        kw = dict(cfg=small_cfg(capi), devices=devices, gate_reference="anchor", gate_settle=(SETTLE, NEVER), group_gate_order="chain")
        rep = matching.ProgressReporter(lambda a, b, c: None)
        vm = matching.HipImageVideoMatcher(**kw).create_video_matcher(objs, rep)
        assert vm._m.gate_order() == "chain" and vm._m.gate_reference() == "anchor" and len(vm._m.devices) == len(devices)
        got = vm.match_images_with_video(video, rep).process()
        out[len(devices)] = [(mm.video_time, mm.video_frame_idx, None if mm.image is None else mm.image.page_nr) for mm in got]
    assert len(out[1]) > 2 and out[1] == out[2]
    with pytest.raises(capi.SlideoError) as e:                   # with the default order the refusal still surfaces when the group is built
        matching.HipImageVideoMatcher(cfg=small_cfg(capi), devices=[0, 0], gate_reference="anchor").create_video_matcher(
            [], matching.ProgressReporter(lambda *a: None))
    assert e.value.code == 5
