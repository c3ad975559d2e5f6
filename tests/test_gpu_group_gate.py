"""The changed-frame gate on an N-device group and the frame-primed gate state (include/slideo_amd.h "Changed-frame gate", the
group's form; slideo_matcher_gate_reset_from_frame_*).  The reference is always a single Matcher of the same config, pages and
options making the same sequence of gate_reset / match_changed_frames calls; every comparison is exact equality of bytes: flags,
similarities (as uint32), verdict records, every candidate trace, the last small image.  Groups are devices=[0] * members, as in
tests/test_gpu_group.py: every control-flow path of an N-GPU node except the second physical device.

Sequences (`_holds`) are lecture-like: a synthetic frame is held for a few frames — each repeat with fresh noise of at most +-2
per byte, a similarity of about 0.997 against the 0.98 that counts as changed — then the next frame follows.  `_boundaries` lists
the first frame of every shard after a call's first; the sequences are built so that these fall alternately inside a hold (the
shard's first frame must come out UNCHANGED: what a group without the halo frame fails) and on a change, and `_conditions` asserts
both from the single matcher's flags before anything is compared."""
import os

import numpy as np
import pytest

import yuv420_ref as yref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

UNCHANGED = (-1, 0.0, 0, 0)


def _shard(n, r, world):
    base, rem = divmod(n, world)
    lo = r * base + min(r, rem)
    return lo, lo + base + (1 if r < rem else 0)


def _boundaries(cuts, members):
    """Global index of the first frame of every non-empty shard after the first, over the calls [cuts[i], cuts[i + 1])."""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        for r in range(1, members):
            lo, hi = _shard(b - a, r, members)
            if hi > lo:
                out.append(a + lo)
    return out


def _holds(base, n, rng, inside=(), on_change=(), lens=(1, 6)):
    """n frames: holds of base[0], base[1], ... (cyclic) with random lengths in [lens[0], lens[1]); the frames `inside` lie inside
    a hold and the frames `on_change` start one.  -> (frames, starts)"""
    starts, i = {0}, 0
    while True:
        i += int(rng.integers(*lens))
        if i >= n:
            break
        starts.add(i)
    starts = sorted((starts | set(on_change)) - set(inside))
    seq = np.empty((n,) + base.shape[1:], np.uint8)
    for j, s in enumerate(starts):
        e = starts[j + 1] if j + 1 < len(starts) else n
        seq[s] = base[j % len(base)]
        for t in range(s + 1, e):
            seq[t] = np.clip(seq[s].astype(np.int16) + rng.integers(-2, 3, seq[s].shape), 0, 255).astype(np.uint8)
    return seq, np.array(starts)


def _sequence(base, n, cuts, members, seed):
    b = _boundaries(cuts, members)
    return _holds(base, n, np.random.default_rng(seed), inside=b[0::2], on_change=b[1::2]) + (b,)


def _single(capi, pages, cfg=None):
    m = capi.Matcher(cfg if cfg is not None else small_cfg(capi))
    m.add_pages(list(pages)); m.finalize()
    return m


def _group(capi, pages, members, cfg=None):
    g = capi.Group(cfg if cfg is not None else small_cfg(capi), devices=[0] * members)
    g.add_pages(list(pages)); g.finalize()
    return g


def _call(h, frames, yuv=None):
    """One gated call on a Matcher or a Group -> (changed, sims, verdicts, traces of the changed frames)."""
    if yuv is None:
        ch, sims, v = h.match_changed_frames(frames)
    else:
        ch, sims, v = h.match_changed_frames_yuv420(frames, *yuv)
    return ch, sims, v, [h.last_candidates(k).tobytes() for k in range(int(ch.sum()))]


def _same(ref, got, what):
    ch, sims, v, tr = got
    assert np.array_equal(ch, ref[0]), (what, "flags", np.nonzero(ch != ref[0])[0][:8])
    assert np.array_equal(sims.view(np.uint32), ref[1].view(np.uint32)), (what, "similarities")
    assert v.tobytes() == ref[2].tobytes(), (what, "verdicts", [i for i in range(len(v)) if v[i] != ref[2][i]][:8])
    assert len(tr) == len(ref[3]), (what, "trace count")
    for k, (a, b) in enumerate(zip(tr, ref[3])):
        assert a == b, (what, "trace of changed frame %d" % k)
    for i in np.nonzero(~ch)[0]:
        assert tuple(v[i]) == UNCHANGED, (what, i)


def _run(m, g, seq, cuts, yuv=None, check_calls=True):
    """The calls [cuts[i], cuts[i + 1]) on the single matcher and on the group; -> the single matcher's flags over the sequence."""
    members = len(g.devices)
    flags = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ref = _call(m, seq[a:b], yuv)
        if check_calls and members > 1:
            assert 0 < int(ref[0].sum()) < b - a, "call %d..%d: some frame changed and some did not (%d of %d)" % (a, b, ref[0].sum(), b - a)
        _same(ref, _call(g, seq[a:b], yuv), "members %d call %d..%d" % (members, a, b))
        flags.append(ref[0])
    if len(flags) and sum(len(f) for f in flags):
        assert np.array_equal(g.gate_last_small(), m.gate_last_small()), "last small image, members %d" % members
    return np.concatenate(flags) if flags else np.zeros(0, bool)


def _conditions(flags, starts, bounds):
    """On the SINGLE matcher's flags: every hold starts with a changed frame and nothing else is changed; a shard's first frame
    inside a hold is unchanged (the frame before its block was compared), and one that starts a hold is changed."""
    want = np.zeros(len(flags), bool)
    want[starts] = True
    assert np.array_equal(flags, want), np.nonzero(flags != want)[0][:8]
    if bounds:
        assert len(bounds) >= 2
        assert (~flags[bounds]).any(), "a shard boundary inside a hold: its first frame is unchanged"
        assert flags[bounds].any(), "a shard boundary on a change"
        assert (~flags[bounds[0::2]]).all() and flags[bounds[1::2]].all()


# ---- the gate state from a frame -----------------------------------------------------------------------------------------------

def _primed_equals_reset(m, r, seq, prime, small_of, call):
    """prime(m, frame 5) against r's gate_reset(small image of frame 5), then the same gated call on both."""
    S = small_of(5)
    prime(5)
    assert np.array_equal(m.gate_last_small(), S)
    r.gate_reset(S)
    ref, got = call(r), call(m)
    assert ref[0].any() and not ref[0].all() and not ref[0][0]          # frame 6 repeats frame 5: compared against S, unchanged
    _same(ref, got, "after the prime")
    assert np.array_equal(m.gate_last_small(), r.gate_last_small())
    # a prime in the middle of a gated sequence replaces the state and forgets the frames seen (as gate_reset does)
    prime(5)
    assert np.array_equal(m.gate_last_small(), S)


@pytest.fixture(scope="module")
def held(cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq, starts = _holds(frames, 20, np.random.default_rng(77), inside=(6,), on_change=(5, 9), lens=(2, 5))
    return pages, seq, starts


def test_prime_bgr_host_and_device(capi, held):
    import torch
    pages, seq, _ = held
    n, h, w, _ = seq.shape
    m, r = _single(capi, pages), _single(capi, pages)
    small_of = lambda i: r.changed_mask(seq[i:i + 1])[2]
    call = lambda x: _call(x, seq[6:16])
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame(seq[i]), small_of, call)
    d = torch.from_numpy(seq).cuda()
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame_dev(d.data_ptr() + i * w * h * 3, w, h), small_of, call)
    # a pitched device frame
    stride = w * 3 + 21
    buf = np.random.default_rng(3).integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w * 3] = seq[5].reshape(h, w * 3)
    dp = torch.from_numpy(buf).cuda()
    m.gate_reset(None)
    m.gate_reset_from_frame_dev(dp.data_ptr(), w, h, stride)
    assert np.array_equal(m.gate_last_small(), small_of(5))
    m.close(); r.close()


def test_prime_nv12_pitched_host_and_device(capi, held):
    import torch
    pages, seq, _ = held
    n, h, w, _ = seq.shape
    L, fb = capi.yuv420_layout("nv12", w, h, pitch=704, row_align=16)
    yuv = yref.frames_to_yuv(seq, L, fb)
    m, r = _single(capi, pages), _single(capi, pages)
    small_of = lambda i: r.changed_mask_yuv420(yuv[i:i + 1], w, h, L)[2]
    call = lambda x: _call(x, yuv[6:16], (w, h, L))
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame_yuv420(yuv[i], w, h, L), small_of, call)
    d = torch.from_numpy(yuv).cuda()
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame_yuv420_dev(d.data_ptr() + i * fb, w, h, L), small_of, call)
    m.close(); r.close()


def test_prime_under_a_working_size(capi, held):
    import torch
    pages, seq, _ = held
    n, h, w, _ = seq.shape
    m, r = _single(capi, pages), _single(capi, pages)
    m.set_working_size(512, 288); r.set_working_size(512, 288)
    small_of = lambda i: r.changed_mask(seq[i:i + 1])[2]
    assert small_of(5).shape[:2] == capi.small_size(512, 288, m.cfg.small_area)[::-1]      # the REDUCED image's small image
    call = lambda x: _call(x, seq[6:16])
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame(seq[i]), small_of, call)
    d = torch.from_numpy(seq).cuda()
    _primed_equals_reset(m, r, seq, lambda i: m.gate_reset_from_frame_dev(d.data_ptr() + i * w * h * 3, w, h), small_of, call)
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = yref.frames_to_yuv(seq, L, fb)
    m.gate_reset_from_frame_yuv420(yuv[5], w, h, L)
    assert np.array_equal(m.gate_last_small(), r.changed_mask_yuv420(yuv[5:6], w, h, L)[2])
    m.close(); r.close()


def test_prime_errors_leave_the_state_untouched(capi, held):
    pages, seq, _ = held
    n, h, w, _ = seq.shape
    m = _single(capi, pages)
    m.gate_reset_from_frame(seq[0])
    S = m.gate_last_small()
    L = capi.yuv420_layout("nv12", w, h)[0]
    bad_layout = capi.yuv420_layout("nv12", w, h)[0]
    bad_layout.y_stride = w - 2
    for bad, code in ((lambda: m.gate_reset_from_frame_yuv420(np.zeros(w * h * 3 // 2, np.uint8), w - 1, h, L), 5),       # odd width: SLIDEO_ERR_UNSUPPORTED
                      (lambda: m.gate_reset_from_frame_yuv420(np.zeros(w * h * 3 // 2, np.uint8), w, h, bad_layout), 1),
                      (lambda: m.gate_reset_from_frame_dev(0, w, h), 1),                                                 # null frame
                      (lambda: m.gate_reset_from_frame_dev(1 << 20, w, h, stride=w), 1)):                                # stride < 3w
        with pytest.raises(capi.SlideoError) as e:
            bad()
        assert e.value.code == code
        assert np.array_equal(m.gate_last_small(), S)
    m.close()


# ---- group == single matcher ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [(0, 17, 30), (0, 11, 19, 30)])
@pytest.mark.parametrize("members", [1, 2, 3, 5])
def test_group_equals_single_matcher(capi, cfg0_data, members, cuts):
    pages, frames, _, _ = cfg0_data
    seq, starts, bounds = _sequence(frames, cuts[-1], cuts, members, seed=100 + members)
    m, g = _single(capi, pages), _group(capi, pages, members)
    for h in (m, g):
        h.gate_reset(None)
    log = []
    g.set_progress(lambda d, t, msg: log.append((d, t)))
    flags = _run(m, g, seq, cuts)
    g.set_progress(None)
    _conditions(flags, starts, bounds)
    # progress covers the frames of each call (a halo frame is not counted), and never decreases within one
    ends = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    assert [t for d, t in log if d == t] == ends
    assert all(d2 >= d1 or t2 != t1 for (d1, t1), (d2, t2) in zip(log[:-1], log[1:]))
    # the whole sequence again as ONE call after a reset: other shard boundaries, the same flags
    for h in (m, g):
        h.gate_reset(None)
    again = _run(m, g, seq, (0, cuts[-1]))
    assert np.array_equal(again, flags)
    m.close(); g.close()


@pytest.mark.parametrize("members", [3, 5])
def test_reset_with_a_small_image_and_short_calls(capi, cfg0_data, members):
    """A reset with a prev_small; then n = 1, n = 0 and n < members beside ordinary calls."""
    pages, frames, _, _ = cfg0_data
    cuts = (0, 12, 13, 13, 15, 30)                              # 12 frames, ONE frame, NO frame, two frames (fewer than members), 15
    bounds = [b for b in _boundaries(cuts, members)]
    seq, starts = _holds(frames, 30, np.random.default_rng(5 + members), inside=[12, 14] + bounds[0::2], on_change=[13] + bounds[1::2], lens=(2, 5))
    starts = starts[starts > 0]
    m, g = _single(capi, pages), _group(capi, pages, members)
    prev = m.changed_mask(seq[:1])[2]                           # frame 0's small image: frame 0 then compares as unchanged
    for h in (m, g):
        h.gate_reset(prev)
        assert np.array_equal(h.gate_last_small(), prev)
    flags = _run(m, g, seq, cuts, check_calls=False)
    assert not flags[0] and 0 < flags.sum() < len(flags)
    assert not flags[12] and flags[13] and not flags[14]        # the one-frame call inside a hold, the two-frame call on a change
    want = np.zeros(30, bool); want[starts] = True
    assert np.array_equal(flags, want)
    for h in (m, g):                                            # n == 0: a no-op; the state stays
        S = h.gate_last_small()
        ch, sims, v = h.match_changed_frames(seq[:0])
        assert len(ch) == len(sims) == len(v) == 0
        assert np.array_equal(h.gate_last_small(), S)
    m.close(); g.close()


def test_yuv420_form(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    cuts, members = (0, 17, 30), 3
    seq, starts, bounds = _sequence(frames, 30, cuts, members, seed=31)
    h, w = seq.shape[1:3]
    L, fb = capi.yuv420_layout("nv12", w, h, pitch=704, row_align=16)
    yuv = yref.frames_to_yuv(seq, L, fb)
    m, g = _single(capi, pages), _group(capi, pages, members)
    flags = _run(m, g, yuv, cuts, yuv=(w, h, L))
    _conditions(flags, starts, bounds)
    m.close(); g.close()


@pytest.mark.parametrize("mode", ["page_set", "working_size", "verify_model_1"])
def test_member_options(capi, cfg0_data, mode):
    pages, frames, _, _ = cfg0_data
    cuts, members = (0, 17, 30), 3
    seq, starts, bounds = _sequence(frames, 30, cuts, members, seed=41)
    cfg = (lambda: small_cfg(capi, verify_model=1)) if mode == "verify_model_1" else (lambda: small_cfg(capi))
    m, g = _single(capi, pages, cfg()), _group(capi, pages, members, cfg())
    if mode == "page_set":
        for h in (m, g):
            h.use_page_set(h.create_page_set([0, 2]))
    if mode == "working_size":
        g.gate_reset(m.changed_mask(seq[:1])[2])
        for h in (m, g):
            h.set_working_size(512, 288)                        # resets the gate state, the group's too
        with pytest.raises(capi.SlideoError) as e:
            g.gate_last_small()
        assert e.value.code == 4
    flags = _run(m, g, seq, cuts)
    _conditions(flags, starts, bounds)
    m.gate_reset(None)
    v = m.match_changed_frames(seq)[2]
    assert (v["page_idx"] >= 0).any(), "the reference assigns a page to some changed frame"
    if mode == "page_set":
        assert set(v["page_idx"].tolist()) <= {-1, 0, 2}
    if mode == "working_size":
        assert g.gate_last_small().shape[:2] == capi.small_size(512, 288, m.cfg.small_area)[::-1]
    m.close(); g.close()


@pytest.mark.parametrize("seed", range(8))
def test_group_gate_random_shards(capi, synth, seed):
    """A seeded sweep, after tests/test_gpu_group.py test_group_random_shards: random hold lengths, member count and call cuts
    (calls of four frames and more, so that holds of two to four frames leave a changed and an unchanged frame in every call)."""
    rng = np.random.default_rng(7300 + seed)
    members = int(rng.integers(2, 6))
    pages = synth.pages(int(rng.integers(2, 6)), 800, 450, seed=int(rng.integers(1, 1 << 30)))
    base, _, _ = synth.frames(pages, 6, 640, 360, seed=int(rng.integers(1, 1 << 30)))
    n = int(rng.integers(12, 40))
    cuts = [0]
    while n - cuts[-1] >= 8 and len(cuts) < 3:
        cuts.append(cuts[-1] + int(rng.integers(4, n - cuts[-1] - 3)))
    cuts.append(n)
    seq, starts = _holds(base, n, rng, lens=(2, 5))
    cfg = small_cfg(capi, nfeatures=int(rng.choice([200, 500])))
    m, g = _single(capi, pages, cfg), _group(capi, pages, members, cfg)
    if rng.integers(0, 2):
        prev = m.changed_mask(seq[int(rng.integers(0, n)):][:1])[2]
        m.gate_reset(prev); g.gate_reset(prev)
    flags = _run(m, g, seq, tuple(cuts))
    assert 0 < flags.sum() < n
    m.close(); g.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_groups_state_untouched(capi, synth, cfg0_data):
    pages, frames, _, _ = cfg0_data
    cuts, members = (0, 10, 30), 3
    seq, starts, bounds = _sequence(frames, 30, cuts, members, seed=51)
    m, g = _single(capi, pages), _group(capi, pages, members)
    with pytest.raises(capi.SlideoError) as e:
        g.gate_last_small()                                      # the state "none"
    assert e.value.code == 4
    f1 = _run(m, g, seq, (0, 10))
    other = synth.frames(pages, 4, 800, 450)[0]
    h, w = seq.shape[1:3]
    L, fb = capi.yuv420_layout("nv12", w, h)
    S = g.gate_last_small()
    for bad, code in ((lambda: g.match_changed_frames(other), 4),                                                      # another size
                      (lambda: g.match_changed_frames_yuv420(yref.frames_to_yuv(seq[:4], L, fb), w, h, L), 4),        # another family
                      (lambda: g.match_changed_frames(np.zeros((4, 0, 4, 3), np.uint8)), 1)):                          # an argument error
        with pytest.raises(capi.SlideoError) as e:
            bad()
        assert e.value.code == code
        assert np.array_equal(g.gate_last_small(), S)
    # the next valid call behaves as if the refused ones had not been made: the single matcher never made them
    f2 = _run(m, g, seq[10:], (0, 20))
    _conditions(np.concatenate([f1, f2]), starts, bounds)
    g.gate_reset(None)
    with pytest.raises(capi.SlideoError) as e:
        g.gate_last_small()
    assert e.value.code == 4
    with pytest.raises(capi.SlideoError) as e:                   # a small image larger than small_area
        g.gate_reset(np.zeros((400, 400, 3), np.uint8))
    assert e.value.code == 1
    ch = g.match_changed_frames(other)[0]                        # after the reset another size is fine, and its first frame is changed
    assert ch[0]
    m.close(); g.close()


# ---- the mirror -----------------------------------------------------------------------------------------------------------------

def test_video_task_gates_on_a_two_member_group(tmp_path, capi, synth, monkeypatch):
    """HipImageVideoMatcher over two members and over one: the same timeline from a raw-video container with holds, through the
    group's gated call and never through the mask call."""
    from PIL import Image
    from slideo_amd import matching as mt

    class Page:
        def __init__(self, path, nr): self.path, self.page_nr = path, nr
        def get_path(self): return self.path
        def __eq__(self, o): return isinstance(o, Page) and o.page_nr == self.page_nr

    pages = synth.pages(4, 800, 450)
    d = os.path.join(tmp_path, "pages"); os.makedirs(d)
    objs = []
    for i, p in enumerate(pages):
        path = os.path.join(d, "p-%d.png" % (i + 1))
        Image.fromarray(np.ascontiguousarray(p[:, :, ::-1])).save(path)
        objs.append(Page(path, i + 1))
    base, _, _ = synth.frames(pages, 8, 640, 360)
    seq, starts = _holds(base, 150, np.random.default_rng(9), inside=(64, 128), lens=(2, 7))      # calls of 64 (one member) and 128 (two)
    vid = os.path.join(tmp_path, "v.slvf")
    mt.RawVideo.write(vid, seq, fps=0.2)                         # one sample per frame
    counts = {"gated": 0, "mask": 0}
    gated, mask = capi.Group.match_changed_frames, capi.Group.changed_mask

    def count_gated(self, frames):
        counts["gated"] += 1
        return gated(self, frames)

    def count_mask(self, frames, prev_small=None):
        counts["mask"] += 1
        return mask(self, frames, prev_small)

    monkeypatch.setattr(capi.Group, "match_changed_frames", count_gated)
    monkeypatch.setattr(capi.Group, "changed_mask", count_mask)
    cfg = capi.default_config(nfeatures=500, min_rating=12.0)
    outs, calls = [], []
    for devs in ([0], [0, 0]):
        counts["gated"] = counts["mask"] = 0
        rep = mt.ProgressReporter(lambda a, b, c: None)
        vm = mt.HipImageVideoMatcher(cfg, devices=devs).create_video_matcher(objs, rep)
        assert mt._gated_matcher(vm._m) is vm._m and len(vm._m.devices) == len(devs)
        out = vm.match_images_with_video(vid, rep).process()
        outs.append([(mm.video_time, mm.video_frame_idx, None if mm.image is None else mm.image.page_nr) for mm in out])
        calls.append(dict(counts))
    assert calls[0] == {"gated": 3, "mask": 0} and calls[1] == {"gated": 2, "mask": 0}, calls
    assert outs[0] == outs[1] and len(outs[0]) > 8 and any(nr is not None for _, _, nr in outs[0])
