"""The levels histogram (include/slideo_amd.h "Frame levels", the learner) on the GPU: levels_hist_kernel against np.bincount of the
analysed images — n in {1, 4, 5, 9} (the frame walk's unrolled part and its tail), one call against the same frames over two calls,
a constant picture (every sample in one bin), two constants alternating (every run breaks), a static picture (one run per
dword), noise; ragged widths; host and device frames, both doors, under a working size; and beside the activity and the content
session, whose counts must be what they are alone.  Exact integers: every comparison is equality."""
import numpy as np
import pytest

import levels_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

NS = [1, 4, 5, 9]


@pytest.fixture(scope="module")
def m(capi):
    x = capi.Matcher(small_cfg(capi))
    yield x
    x.close()


def _contents(name, n, h, w, frame, seed):
    rng = np.random.default_rng(seed)
    if name == "white":
        return np.full((n, h, w, 3), 255, np.uint8)
    if name == "alternating":
        f = np.empty((n, h, w, 3), np.uint8)
        f[0::2] = (12, 200, 90); f[1::2] = (13, 200, 91)
        return f
    if name == "static":
        return np.ascontiguousarray(np.repeat(frame[None, :h, :w], n, axis=0))
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _hist(m, feed):
    m.levels_begin()
    try:
        feed()
        return m.levels_histogram(), m.levels_info()
    finally:
        m.levels_end()


@pytest.mark.parametrize("name", ["white", "alternating", "static", "noise"])
def test_histogram_equals_bincount(capi, m, cfg0_data, name):
    frame = cfg0_data[1][1]
    for k, (w, h) in enumerate(((640, 360), (61, 47), (130, 33))):
        for n in NS:
            frames = _contents(name, n, h, w, frame, 10 * k + n)
            want = R.histogram(frames)
            got, info = _hist(m, lambda: m.observe_frames(frames))
            assert np.array_equal(got, want), (name, w, h, n)
            assert info == {"frames": n, "pixels": n * w * h}
            if n > 1:                                             # the same frames over two calls
                got2, info2 = _hist(m, lambda: (m.observe_frames(frames[:n // 2]), m.observe_frames(frames[n // 2:])))
                assert np.array_equal(got2, want) and info2 == info
    if name == "white":
        assert want[:, 255].tolist() == [9 * 130 * 33] * 3 and int(want.sum()) == 3 * 9 * 130 * 33


def test_frames_of_different_sizes_add_up(m):
    a = np.random.default_rng(1).integers(0, 256, (2, 47, 61, 3), dtype=np.uint8)
    b = np.random.default_rng(2).integers(0, 256, (3, 33, 130, 3), dtype=np.uint8)
    got, info = _hist(m, lambda: (m.observe_frames(a), m.observe_frames(b)))
    assert np.array_equal(got, R.histogram(a) + R.histogram(b))
    assert info == {"frames": 5, "pixels": 2 * 47 * 61 + 3 * 33 * 130}


def test_device_frames_at_any_alignment(m, cfg0_data):
    import torch
    frames = np.ascontiguousarray(np.repeat(cfg0_data[1][:3], 3, axis=0)[:5, :47, :130])
    n, h, w, _ = frames.shape
    want = R.histogram(frames)
    for ofs, extra, slack in ((0, 0, 0), (1, 0, 0), (2, 1, 3), (0, 2, 4)):
        stride = 3 * w + extra
        fs = h * stride + slack
        host = np.random.default_rng(ofs).integers(0, 256, n * fs, dtype=np.uint8)
        for i in range(n):
            host[i * fs: i * fs + h * stride].reshape(h, stride)[:, :3 * w] = frames[i].reshape(h, 3 * w)
        t = torch.empty(ofs + host.size, dtype=torch.uint8, device="cuda")
        t[ofs:].copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        got, _ = _hist(m, lambda: m.observe_frames_dev(t.data_ptr() + ofs, n, w, h, stride, fs))
        assert np.array_equal(got, want), (ofs, extra, slack)
        assert np.array_equal(t[ofs:].cpu().numpy(), host)


def test_the_yuv_door_and_a_working_size(capi, m, cfg0_data):
    frames = cfg0_data[1][:4]
    n, h, w, _ = frames.shape
    L, fb = capi.yuv420_layout("nv12", w, h)
    yuv = np.random.default_rng(3).integers(16, 236, (3, fb), dtype=np.uint8)
    imgs = np.stack([m.yuv420_to_bgr(yuv[i], w, h, L) for i in range(3)])
    got, info = _hist(m, lambda: m.observe_frames_yuv420(yuv, w, h, L))
    assert np.array_equal(got, R.histogram(imgs)) and info["pixels"] == 3 * w * h
    m.set_working_size(480, 270)
    try:
        red = np.stack([m.reduce(f, 480, 270) for f in frames])
        got, info = _hist(m, lambda: m.observe_frames(frames))
        assert np.array_equal(got, R.histogram(red)) and info == {"frames": 4, "pixels": 4 * 480 * 270}
    finally:
        m.set_working_size(0, 0)


def test_beside_the_activity_and_content_sessions(m, cfg0_data):
    frames = np.ascontiguousarray(np.repeat(cfg0_data[1][:4], 2, axis=0))
    m.activity_begin(12); m.content_begin(24)
    m.observe_frames(frames[:3]); m.observe_frames(frames[3:])
    act, cnt = m.activity_counts(), m.content_counts()
    m.activity_end(); m.content_end()
    m.activity_begin(12); m.content_begin(24); m.levels_begin()
    m.observe_frames(frames[:3]); m.observe_frames(frames[3:])
    act2, cnt2, hist = m.activity_counts(), m.content_counts(), m.levels_histogram()
    # the other two end first: the levels session still holds what it counted, and goes on alone
    m.activity_end(); m.content_end()
    assert np.array_equal(m.levels_histogram(), hist)
    m.observe_frames(frames[:1])
    assert np.array_equal(m.levels_histogram(), R.histogram(frames) + R.histogram(frames[:1]))
    m.levels_end()
    assert np.array_equal(act2[0], act[0]) and act2[1] == act[1] and np.array_equal(cnt2[0], cnt[0]) and cnt2[1] == cnt[1]
    assert np.array_equal(hist, R.histogram(frames))
