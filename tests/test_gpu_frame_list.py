"""Frame lists (include/slideo_amd.h "Frame lists") on the GPU: every list call returns, bit for bit, what the contiguous call of the
same family returns for frames holding the same samples.  The tap over the host check's matrix (tools/frame_list_hostcheck.cpp) in
host and device memory; every call form against its contiguous twin over nine format forms on the cfg0 deck and its 640x360 frames;
the default path before and after list calls; the refusals on a live matcher.  All comparisons are byte equality."""
import ctypes as C

import numpy as np
import pytest

import pixel_format_ref as PR
import yuv_desc_ref as YD
import yuv_sampling_ref as YS
import yuv_transfer_ref as YT
from conftest import small_cfg

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _same3(a, b):
    """(changed, similarity, verdicts) of two gated calls."""
    return np.array_equal(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


def _code(capi, fn):
    with pytest.raises(capi.SlideoError) as e:
        fn()
    return e.value.code, str(e.value)


# ---- a format form: the settings it is read under, its contiguous frames and the planes of one frame ----------------------------------

class Form:
    """door "bgr": fmt is a pixel format name; door "yuv": a YUV format name read under (matrix, range, depth) and a transfer."""

    def __init__(self, name, door, fmt, depth="8", matrix="bt601", rng="limited", transfer=None):
        self.name, self.door, self.fmt, self.depth, self.matrix, self.rng, self.transfer = name, door, fmt, depth, matrix, rng, transfer
        self.bps = 1 if depth == "8" else 2

    def apply(self, capi, x):
        x.set_yuv_transfer("sdr")
        x.set_yuv_description()
        x.set_yuv_sampling("420")
        x.set_pixel_format("bgr")
        if self.door == "bgr":
            x.set_pixel_format(self.fmt)
            return
        x.set_yuv_sampling(capi.yuv_format_sampling(self.fmt))
        x.set_yuv_description(self.matrix, self.rng, self.depth)
        if self.transfer:
            x.set_yuv_transfer(self.transfer, 0)

    def layout(self, capi, w, h):
        return capi.yuv_layout(self.fmt, w, h, bytes_per_sample=self.bps)

    def encode(self, capi, seq):
        """BGR images [n, h, w, 3] -> tight contiguous frames [n, frame bytes] of the form that stand for (about) those images."""
        n, h, w, _ = seq.shape
        if self.door == "bgr":
            return seq.reshape(n, -1) if self.fmt == "bgr" else np.stack([PR.pack(seq[i], self.fmt, seed=i) for i in range(n)])
        L, fb = self.layout(capi, w, h)
        depth = capi.YUV_DEPTHS[self.depth]
        sampling = capi.YUV_SAMPLINGS[capi.yuv_format_sampling(self.fmt)]
        if self.transfer:
            return YT.frames_to_yuv(seq, L, fb, capi.YUV_TRANSFERS[self.transfer], capi.YUV_RANGES[self.rng], depth, sampling, 0)
        desc = (capi.YUV_MATRICES[self.matrix], capi.YUV_RANGES[self.rng], depth)
        return YD.frames_to_yuv(seq, L, fb, desc) if sampling == YS.S420 else YS.frames_to_yuv(seq, L, fb, desc, sampling)

    def random(self, capi, w, h, n, seed):
        """n tight frames of random bytes (every byte a sample or ignored: the tap compares conversions of the same bytes)."""
        fb = w * h * 3 if self.fmt == "bgr" else PR.span(self.fmt, w, h, w * PR.info(self.fmt)[0]) if self.door == "bgr" else self.layout(capi, w, h)[1]
        return np.random.default_rng(seed).integers(0, 256, (n, fb), dtype=np.uint8)

    def planes(self, capi, frame, w, h):
        """The planes of one tight frame as 2-D byte views [rows, row bytes], and the `chroma` argument of capi.frame_list."""
        if self.door == "bgr":
            bpp, planes = (3, 1) if self.fmt == "bgr" else PR.info(self.fmt)
            return [frame[k * h * w * bpp: (k + 1) * h * w * bpp].reshape(h, w * bpp) for k in range(planes)], None
        L, _ = self.layout(capi, w, h)
        sampling = capi.yuv_format_sampling(self.fmt)
        if sampling == "422_packed":
            return [frame.reshape(h, 2 * w)], self.fmt
        b = self.bps
        cw, ch = (w if sampling == "444" else w // 2), (h // 2 if sampling == "420" else h)
        Y = frame[: h * w * b].reshape(h, w * b)
        if L.uv_step == 2:
            lo = min(L.u_offset, L.v_offset)
            return [Y, frame[lo: lo + ch * cw * 2 * b].reshape(ch, cw * 2 * b)], ("uv" if L.u_offset < L.v_offset else "vu")
        return [Y] + [frame[o: o + ch * cw * b].reshape(ch, cw * b) for o in (L.u_offset, L.v_offset)], None

    def contiguous(self, capi, m, name, flat, w, h, *extra):
        """The contiguous twin of a host call: m.<name>(frames ...) through the form's door."""
        if self.door == "bgr":
            arr = flat.reshape(-1, h, w, 3) if self.fmt == "bgr" else PR.as_array(flat, self.fmt, w, h)
            return getattr(m, name)(arr, *extra)
        return getattr(m, name + "_yuv420")(flat, w, h, self.layout(capi, w, h)[0], *extra)


FORMS = [Form("bgr8", "bgr", "bgr"), Form("rgba", "bgr", "rgba"), Form("planar_rgb", "bgr", "planar_rgb"), Form("nv12", "yuv", "nv12"),
         Form("i420", "yuv", "i420"), Form("p010", "yuv", "nv12", "10_msb", "bt709", "limited"), Form("uyvy", "yuv", "uyvy"),
         Form("i444", "yuv", "i444"), Form("p010_hlg", "yuv", "nv12", "10_msb", "bt709", "limited", "hlg")]


def _scatter(capi, form, flat, w, h, device, pads=(0, 0, 0), ofs=None):
    """A frame list of the tight frames `flat`: every plane of every frame in its own allocation (its rows pads[k] bytes beyond tight,
    its first byte ofs[i] bytes past the allocation's base), the frames allocated in reverse order with unequal gaps between them."""
    import torch
    n = len(flat)
    frames, junk = [None] * n, []
    for i in reversed(range(n)):
        pl, chroma = form.planes(capi, flat[i], w, h)
        o = 0 if ofs is None else ofs[i]
        out = []
        for k, p in enumerate(pl):
            rows, rb = p.shape
            size = o + rows * (rb + pads[k])
            buf = torch.empty(size, dtype=torch.uint8, device="cuda") if device else np.empty(size, np.uint8)
            v = buf[o: o + rows * (rb + pads[k])].reshape(rows, rb + pads[k])[:, :rb]
            if device:
                v.copy_(torch.from_numpy(np.ascontiguousarray(p)))
            else:
                v[...] = p
            out.append(v)
        junk.append(torch.empty(256 * (1 + i % 3), dtype=torch.uint8, device="cuda") if device else np.empty(64 * (1 + i % 3), np.uint8))
        frames[i] = tuple(out) if len(out) > 1 else out[0]
    if device:
        torch.cuda.synchronize()
    fl = capi.frame_list(frames, form.door, w, h, chroma=chroma, planar=form.door == "bgr" and len(pl) == 3, bps=form.bps)
    fl.junk = junk
    return fl


# ---- 1. the tap over the host check's matrix ---------------------------------------------------------------------------------------

def _tap_forms():
    out = []
    for fmts, depths in ((("i420", "nv12", "nv21"), ("8", "10_msb", "10_lsb")), (("i422", "nv16", "nv61"), ("8", "10_msb", "10_lsb")),
                         (("i444", "nv24", "nv42"), ("8", "10_msb", "10_lsb")), (("yuy2", "yvyu", "uyvy", "vyuy"), ("8",))):
        out += [Form("%s_%s" % (f, d), "yuv", f, d) for f in fmts for d in depths]
    return out + [Form("bgr8", "bgr", "bgr"), Form("bgra", "bgr", "bgra"), Form("planar_rgb", "bgr", "planar_rgb")]


@pytest.fixture(scope="module")
def tap(capi):
    m = capi.Matcher(small_cfg(capi))
    yield m
    m.close()


def _tap_twin(capi, form, m, frame, w, h):
    if form.door == "yuv":
        return m.yuv420_to_bgr(frame, w, h, form.layout(capi, w, h)[0])
    if form.fmt == "bgr":
        return frame.reshape(h, w, 3)
    return m.pixels_to_bgr(PR.as_array(frame, form.fmt, w, h))


@pytest.mark.parametrize("form", _tap_forms(), ids=lambda f: f.name)
def test_tap_bit_exact_over_the_matrix(capi, tap, form):
    form.apply(capi, tap)
    sizes = [(18, 10), (66, 34)] + ([(17, 9)] if form.door == "bgr" or capi.yuv_format_sampling(form.fmt) == "444" else [])
    offsets = [0, 1, 2, 4, 8, 16] if form.bps == 1 else [0, 2, 4, 8, 16]
    for w, h in sizes:
        flat = form.random(capi, w, h, len(offsets), w * 131 + h)
        want = np.stack([_tap_twin(capi, form, tap, flat[i], w, h) for i in range(len(flat))])
        for device in (False, True):
            for pad in (0, 2):
                fl = _scatter(capi, form, flat, w, h, device, (pad, pad, pad), offsets)
                got = tap.frame_list_to_bgr8(fl)
                assert np.array_equal(got, want), (form.name, w, h, device, pad, np.argwhere(got != want)[:4])
            one = _scatter(capi, form, flat[2:3], w, h, device, (2, 2, 2), [offsets[2]])
            assert np.array_equal(tap.frame_list_to_bgr8(one), want[2:3]), (form.name, w, h, device)
    Form("bgr8", "bgr", "bgr").apply(capi, tap)


# ---- 2. every call form against its contiguous twin ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def deck(capi, cfg0_data):
    pages, frames, _, _ = cfg0_data
    seq = np.ascontiguousarray(np.repeat(frames[:5], 2, axis=0))  # every frame twice: changed and unchanged flags both occur
    return pages, seq


def _matcher(capi, pages, form=None, sift=None):
    m = capi.Matcher(small_cfg(capi))
    if sift is not None:
        m.use_sift(*sift)
    m.add_pages(list(pages))
    m.finalize()
    if form is not None:
        form.apply(capi, m)
    return m


@pytest.fixture(scope="module", params=FORMS, ids=lambda f: f.name)
def pair(request, capi, deck):
    """Two matchers under the form's settings (m takes lists, ref the contiguous calls), the sequence as tight contiguous frames, and
    the same frames as a host list (pitched rows) and a device list (tight rows, odd-sized gaps)."""
    form = request.param
    pages, seq = deck
    n, h, w, _ = seq.shape
    flat = form.encode(capi, seq)
    m, ref = _matcher(capi, pages, form), _matcher(capi, pages, form)
    host = lambda sel=slice(None): _scatter(capi, form, flat[sel], w, h, False, (6, 2, 2))
    dev = lambda sel=slice(None): _scatter(capi, form, flat[sel], w, h, True)
    yield form, m, ref, flat, host, dev, w, h
    m.close(); ref.close()


def test_match_frames_host_device_and_streaming(capi, pair):
    form, m, ref, flat, host, dev, w, h = pair
    n = len(flat)
    want = form.contiguous(capi, ref, "match_frames", flat, w, h)
    c_want = [ref.last_candidates(i) for i in range(n)]
    assert (want["page_idx"] >= 0).mean() >= 0.5
    for fl in (host(), dev()):
        assert _same(m.match_frames_list(fl), want)
        for i in range(n):
            assert _same(m.last_candidates(i), c_want[i]), "candidate trace of frame %d" % i
    # submit / collect: the caller's planes array is overwritten right after submit; a busy matcher refuses a setter
    lists = [dev(slice(i, i + 4)) for i in range(0, n, 4)]
    tickets = []
    for fl in lists:
        tickets.append(m.submit_list(fl))
        for k in range(len(fl.table)):
            fl.table[k] = 0xDEAD0000
        fl.rec.width = 1
    c, _ = _code(capi, lambda: m.set_working_size(320, 180))
    assert c == 4
    assert _code(capi, lambda: m.match_frames_list(host()))[0] == 4
    got = np.concatenate([m.collect(t) for t in tickets])
    assert _same(got, want)
    # a host list has no submit form
    c, msg = _code(capi, lambda: m.submit_list(host()))
    assert c == 1 and "device lists" in msg


def test_changed_mask_and_kept_frames(capi, pair):
    form, m, ref, flat, host, dev, w, h = pair
    ch, sim, last = form.contiguous(capi, ref, "changed_mask", flat, w, h)
    assert ch.any() and not ch.all()
    kept_want = ref.match_kept_frames([0, 3, 4])
    for fl in (host(), dev()):
        gc, gs, gl = m.changed_mask_list(fl)
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
        assert _same(m.match_kept_frames([0, 3, 4]), kept_want)
    gc2, gs2, gl2 = m.changed_mask_list(host(slice(3, None)), prev_small=gl)
    ch2, sim2, last2 = form.contiguous(capi, ref, "changed_mask", flat[3:], w, h, last)
    assert np.array_equal(gc2, ch2) and _same(gs2, sim2) and np.array_equal(gl2, last2)


@pytest.mark.parametrize("gate", ["previous", "anchor_settle"])
def test_gated_calls(capi, pair, gate):
    form, m, ref, flat, host, dev, w, h = pair
    n = len(flat)
    for x in (m, ref):
        if gate == "anchor_settle":
            x.set_gate_reference("anchor")
            x.set_gate_settle(0.99, 2)
        x.gate_reset()
    try:
        want = [form.contiguous(capi, ref, "match_changed_frames", flat[:5], w, h), form.contiguous(capi, ref, "match_changed_frames", flat[5:], w, h)]
        want_small = ref.gate_last_small()
        want_state = ref.gate_state_export()
        for mk in (host, dev):
            m.gate_reset()
            got = [m.match_changed_frames_list(mk(slice(0, 5))), m.match_changed_frames_list(mk(slice(5, None)))]
            assert _same3(got[0], want[0]) and _same3(got[1], want[1])
            assert np.array_equal(m.gate_last_small(), want_small) and m.gate_state_export() == want_state
        m.gate_reset()
        tickets = [m.submit_changed_list(dev(slice(0, 5))), m.submit_changed_list(dev(slice(5, None)))]
        for tk, wnt in zip(tickets, want):
            assert _same3(m.collect_changed(tk), wnt)
        assert m.gate_state_export() == want_state
        # the state primed from a list of one
        ref.gate_reset()
        form.contiguous(capi, ref, "match_changed_frames", flat[2:3], w, h)
        a = form.contiguous(capi, ref, "match_changed_frames", flat[3:6], w, h)
        for mk in (host, dev):
            m.gate_reset_from_frame_list(mk(slice(2, 3)))
            assert _same3(m.match_changed_frames_list(mk(slice(3, 6))), a)
            assert np.array_equal(m.gate_last_small(), ref.gate_last_small())
        c, msg = _code(capi, lambda: m.gate_reset_from_frame_list(host(slice(0, 2))))
        assert c == 1 and "list of one" in msg
    finally:
        for x in (m, ref):
            x.set_gate_settle(0, 0)
            x.set_gate_reference("previous")
            x.gate_reset()


def test_observe_frames_and_an_evidence_session(capi, pair):
    form, m, ref, flat, host, dev, w, h = pair
    for x in (m, ref):
        x.activity_begin(12)
        x.content_begin(24)
    form.contiguous(capi, ref, "observe_frames", flat[:2], w, h)
    form.contiguous(capi, ref, "observe_frames", flat[2:], w, h)
    m.observe_frames_list(host(slice(0, 2)))
    m.observe_frames_list(dev(slice(2, None)))
    a, b = m.activity_counts(), ref.activity_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == len(flat) - 1 and b[0].any()
    a, b = m.content_counts(), ref.content_counts()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == len(flat)
    for x in (m, ref):
        x.activity_end()
        x.content_end()
    for x in (m, ref):
        x.evidence_begin(32, 8)
    form.contiguous(capi, ref, "match_frames", flat, w, h)
    m.match_frames_list(host(slice(0, 5)))
    m.match_frames_list(dev(slice(5, None)))
    a, b = m.evidence_counts(), ref.evidence_counts()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:] and b[0].any()
    for x in (m, ref):
        x.evidence_end()


def test_group_of_two_members(capi, pair, deck):
    form, m, ref, flat, host, dev, w, h = pair
    want = form.contiguous(capi, ref, "match_frames", flat, w, h)
    ch, sim, last = form.contiguous(capi, ref, "changed_mask", flat, w, h)
    kept = ref.match_kept_frames([1, 2, 9])
    ref.gate_reset()
    gated = form.contiguous(capi, ref, "match_changed_frames", flat, w, h)
    ref.gate_reset()
    g = capi.Group(small_cfg(capi), [0, 0])
    g.add_pages(list(deck[0]))
    g.finalize()
    form.apply(capi, g)
    fl = host()
    assert _same(g.match_frames_list(fl), want)
    gc, gs, gl = g.changed_mask_list(fl)
    assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    assert _same(g.match_kept_frames([1, 2, 9]), kept)
    assert _same3(g.match_changed_frames_list(fl), gated)
    c, msg = _code(capi, lambda: g.match_frames_list(dev()))
    assert c == 1 and "host lists" in msg
    g.close()


def test_a_list_that_repeats_one_frame(capi, pair):
    form, m, ref, flat, host, dev, w, h = pair
    n = 5
    want = form.contiguous(capi, ref, "match_frames", np.repeat(flat[4:5], n, axis=0), w, h)
    for mk in (host, dev):
        one = mk(slice(4, 5))
        rec = capi.FrameListRec.from_buffer_copy(one.rec)
        table = (C.c_void_p * (3 * n))(*([one.table[k] for k in range(3)] * n))
        rec.n_frames, rec.planes = n, C.cast(table, C.c_void_p)
        assert _same(m.match_frames_list(capi.FrameList(rec, table, one)), want)


# ---- 3. one case each under the other frame settings ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nv12(capi, deck):
    form = FORMS[3]
    pages, seq = deck
    n, h, w, _ = seq.shape
    flat = form.encode(capi, seq)
    m, ref = _matcher(capi, pages, form), _matcher(capi, pages, form)
    host = lambda sel=slice(None): _scatter(capi, form, flat[sel], w, h, False, (6, 2, 2))
    dev = lambda sel=slice(None): _scatter(capi, form, flat[sel], w, h, True)
    yield form, m, ref, flat, host, dev, w, h
    m.close(); ref.close()


def test_under_a_working_size_a_region_levels_and_a_gate_mask(capi, nv12):
    form, m, ref, flat, host, dev, w, h = nv12
    for x in (m, ref):
        x.set_working_size(480, 270)
    try:
        want = form.contiguous(capi, ref, "match_frames", flat[::2], w, h)
        assert _same(m.match_frames_list(host(slice(None, None, 2))), want)
        assert _same(m.match_frames_list(dev(slice(None, None, 2))), want)
        ch, sim, last = form.contiguous(capi, ref, "changed_mask", flat[:6], w, h)
        gc, gs, gl = m.changed_mask_list(dev(slice(0, 6)))
        assert np.array_equal(gc, ch) and _same(gs, sim) and np.array_equal(gl, last)
    finally:
        for x in (m, ref):
            x.set_working_size(0, 0)
    for x in (m, ref):
        x.set_frame_region(w, h, [(40, 30), (w - 41, 24), (w - 37, h - 31), (44, h - 25)], 480, 270)
    try:
        want = form.contiguous(capi, ref, "match_frames", flat[::2], w, h)
        assert _same(m.match_frames_list(host(slice(None, None, 2))), want)
        for x in (m, ref):
            x.gate_reset()
        a = form.contiguous(capi, ref, "match_changed_frames", flat[:6], w, h)
        assert _same3(m.match_changed_frames_list(dev(slice(0, 6))), a)
    finally:
        for x in (m, ref):
            x.clear_frame_region()
            x.gate_reset()
    lut = capi.frame_levels_lut([10, 0, 20], [240, 255, 230])
    for x in (m, ref):
        x.set_frame_levels(lut)
    try:
        want = form.contiguous(capi, ref, "match_frames", flat[::2], w, h)
        assert _same(m.match_frames_list(host(slice(None, None, 2))), want)
        assert _same(m.match_frames_list(dev(slice(None, None, 2))), want)
    finally:
        for x in (m, ref):
            x.set_frame_levels(None)
    mask = np.full((h, w), 255, np.uint8)
    mask[: h // 3, w // 2:] = 0
    for x in (m, ref):
        x.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
        x.set_frame_mask(mask)
        x.gate_reset()
    try:
        a = form.contiguous(capi, ref, "match_changed_frames", flat, w, h)
        assert _same3(m.match_changed_frames_list(dev()), a)
        for i in range(int(a[0].sum())):
            assert _same(m.last_candidates(i), ref.last_candidates(i))
    finally:
        for x in (m, ref):
            x.set_frame_mask(None)
            x.set_frame_mask_scope(capi.MASK_DETECT)
            x.gate_reset()


def test_sift_mode(capi, deck):
    pages, seq = deck
    n, h, w, _ = seq.shape
    form = FORMS[4]                                               # I420, three separately allocated planes
    sift = (capi.sift_config(nfeatures=300), 0.0)
    m, ref = _matcher(capi, pages, form, sift), _matcher(capi, pages, form, sift)
    flat = form.encode(capi, seq[::3])
    want = form.contiguous(capi, ref, "match_frames", flat, w, h)
    assert (want["page_idx"] >= 0).any()
    assert _same(m.match_frames_list(_scatter(capi, form, flat, w, h, True, (0, 2, 2))), want)
    for i in range(len(flat)):
        assert _same(m.last_candidates(i), ref.last_candidates(i))
    m.close(); ref.close()


# ---- 4. the default path, before and after list calls ---------------------------------------------------------------------------------

def test_default_path_is_untouched(capi, deck):
    import torch
    pages, seq = deck
    n, h, w, _ = seq.shape
    form = FORMS[0]
    fresh, m = _matcher(capi, pages), _matcher(capi, pages)
    d = torch.from_numpy(seq).cuda()
    before = (m.match_frames(seq), m.match_frames_dev(d.data_ptr(), n, w, h))
    m.gate_reset()
    before_gated = m.match_changed_frames(seq)
    flat = form.encode(capi, seq)
    m.match_frames_list(_scatter(capi, form, flat, w, h, False, (3, 0, 0)))
    m.match_frames_list(_scatter(capi, form, flat, w, h, True))
    m.gate_reset()
    m.match_changed_frames_list(_scatter(capi, form, flat, w, h, True))
    m.gate_reset()
    after = (m.match_frames(seq), m.match_frames_dev(d.data_ptr(), n, w, h))
    assert _same3(m.match_changed_frames(seq), before_gated)
    want = fresh.match_frames(seq)
    for got in before + after:
        assert _same(got, want)
    m.close(); fresh.close()


# ---- 5. refusals on a live matcher -----------------------------------------------------------------------------------------------------

def test_refusals(capi, pair):
    form, m, ref, flat, host, dev, w, h = pair
    L = capi.lib()
    n = len(flat)
    out = np.zeros(n, capi.VERDICT_DTYPE)
    po = out.ctypes.data_as(C.c_void_p)
    good = host()
    assert L.slideo_match_frames_list(m._h, good.ref(), po, None) == 0
    want = out.copy()

    def refused(edit, code, word):
        rec = capi.FrameListRec.from_buffer_copy(good.rec)
        table = (C.c_void_p * (3 * n))(*[good.table[k] for k in range(3 * n)])
        rec.planes = C.cast(table, C.c_void_p)
        edit(rec, table)
        assert L.slideo_match_frames_list(m._h, C.byref(rec), po, None) == code, word
        assert word in L.slideo_last_error(m._h).decode(), (word, L.slideo_last_error(m._h).decode())

    assert L.slideo_match_frames_list(m._h, None, po, None) == 1 and "null record" in L.slideo_last_error(m._h).decode()
    refused(lambda r, t: setattr(r, "planes", None), 1, "null planes array")
    refused(lambda r, t: t.__setitem__(3, None), 1, "needed and NULL")
    refused(lambda r, t: setattr(r, "door", 7), 1, "door")
    refused(lambda r, t: setattr(r, "on_device", -1), 1, "on_device")
    refused(lambda r, t: r.stride.__setitem__(0, 1), 1, "row bytes")
    refused(lambda r, t: r.stride.__setitem__(0, -r.stride[0]), 1, "negative")
    refused(lambda r, t: setattr(r, "width", 0), 1, "geometry")
    if form.door == "bgr" and form.fmt != "planar_rgb":
        refused(lambda r, t: t.__setitem__(1, t[0]), 1, "not NULL")
    if form.door == "yuv":
        refused(lambda r, t: setattr(r, "uv_step", 3), 1, "uv_step")
        if capi.yuv_format_sampling(form.fmt) != "444":
            refused(lambda r, t: (setattr(r, "width", w - 1), [r.stride.__setitem__(k, r.stride[k] + 8) for k in range(3)]), 5, "even")
    if form.bps == 2:
        refused(lambda r, t: t.__setitem__(0, t[0] + 1), 1, "even addresses")
        refused(lambda r, t: r.stride.__setitem__(0, r.stride[0] + 1), 1, "even strides")
    if form.fmt == "nv12":
        refused(lambda r, t: t.__setitem__(2, t[1] + 2 * form.bps), 1, "interleaved")
    if form.fmt == "uyvy":
        refused(lambda r, t: t.__setitem__(2, t[0] + 3), 1, "(u_offset, v_offset)")
    # every refusal left the matcher as it was
    assert L.slideo_match_frames_list(m._h, good.ref(), po, None) == 0 and _same(out, want)
