"""YUV 4:2:0 front door (include/slideo_amd.h "YUV 4:2:0 frames") without a GPU: the exports, the layout record, the packed
layouts the library computes, and the known answers of the test-side restatement (tests/yuv420_ref.py) the GPU tests compare with."""
import ctypes as C

import numpy as np
import pytest

import yuv420_ref as ref

NEW_SYMBOLS = ["slideo_yuv420_layout_packed", "slideo_match_frames_yuv420", "slideo_match_frames_yuv420_dev",
               "slideo_match_frames_submit_yuv420_dev", "slideo_changed_mask_yuv420", "slideo_yuv420_to_bgr8",
               "slideo_group_match_frames_yuv420", "slideo_group_changed_mask_yuv420"]


def test_library_exports_the_yuv420_symbols(capi):
    L = capi.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in capi.EXPORTS, n


def test_layout_record_matches_the_header(capi):
    T = capi.Yuv420Layout
    assert C.sizeof(T) == 32
    assert [f for f, _ in T._fields_] == ["y_stride", "uv_stride", "u_offset", "v_offset", "uv_step", "_pad"]
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 4, 8, 16, 24, 28]


@pytest.mark.parametrize("w,h", [(640, 360), (1920, 1080), (642, 362), (2, 2), (3840, 2160)])
def test_packed_layouts(capi, w, h):
    n = w * h
    want = {"nv12": (w, w, n, n + 1, 2), "nv21": (w, w, n + 1, n, 2),
            "i420": (w, w // 2, n, n + n // 4, 1), "yv12": (w, w // 2, n + n // 4, n, 1)}
    for fmt, exp in want.items():
        L = capi.yuv420_layout_packed(fmt, w, h)
        assert (L.y_stride, L.uv_stride, L.u_offset, L.v_offset, L.uv_step) == exp, fmt
        P, fb = capi.yuv420_layout(fmt, w, h)                     # the Python helper's tight layout is the library's
        assert bytes(P) == bytes(L) and fb == n * 3 // 2


def test_packed_layout_rejects(capi):
    L = capi.Yuv420Layout()
    f = capi.lib().slideo_yuv420_layout_packed
    assert f(0, 641, 360, C.byref(L)) == 5 and f(2, 640, 361, C.byref(L)) == 5      # odd sides: UNSUPPORTED, as cvtColor
    assert f(4, 640, 360, C.byref(L)) == 1 and f(-1, 640, 360, C.byref(L)) == 1
    assert f(0, 0, 360, C.byref(L)) == 1 and f(0, 640, 360, None) == 1


def test_pitched_layout_helper(capi):
    L, fb = capi.yuv420_layout("nv12", 1920, 1080, pitch=2048, row_align=16)
    assert (L.y_stride, L.uv_stride, L.u_offset, L.v_offset, L.uv_step) == (2048, 2048, 2048 * 1088, 2048 * 1088 + 1, 2)
    assert fb == 2048 * 1088 * 3 // 2
    L, _ = capi.yuv420_layout("yv12", 642, 360, pitch=768, row_align=16)
    assert (L.uv_stride, L.v_offset, L.u_offset) == (384, 768 * 368, 768 * 368 + 384 * 184)


def test_reference_known_answers(capi):
    for fmt in ("nv12", "i420"):
        L, fb = capi.yuv420_layout(fmt, 2, 2)
        for Yv, want in ((16, 0), (235, 255), (0, 0), (255, 255)):
            buf = ref.pack(np.full((2, 2), Yv, np.uint8), np.full((1, 1), 128, np.uint8), np.full((1, 1), 128, np.uint8), L, fb)
            assert (ref.to_bgr(buf, 2, 2, L) == want).all(), (fmt, Yv)
        # nearest chroma: every pixel of a 2 x 2 block takes the block's sample
        Y = np.array([[16, 100], [180, 235]], np.uint8)
        buf = ref.pack(Y, np.array([[200]], np.uint8), np.array([[60]], np.uint8), L, fb)
        got = ref.to_bgr(buf, 2, 2, L).reshape(4, 3).astype(int)
        assert np.abs(got - ref.float_bgr(Y.reshape(4), 200, 60)).max() <= 1


def test_reference_agrees_with_float_bt601():
    g = np.arange(0, 256, 3)
    Y, U, V = np.meshgrid(g, np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
    Y, U, V = Y.reshape(-1), U.reshape(-1), V.reshape(-1)
    u, v = U.astype(np.int64) - 128, V.astype(np.int64) - 128
    y = np.maximum(Y.astype(np.int64) - 16, 0) * ref.CY
    fixed = np.clip(np.stack([(y + ref.HALF + ref.CUB * u) >> 20, (y + ref.HALF + ref.CVG * v + ref.CUG * u) >> 20,
                              (y + ref.HALF + ref.CVR * v) >> 20], -1), 0, 255)
    assert np.abs(fixed - ref.float_bgr(Y, U, V)).max() <= 1
    # the restatement's frame form (here planar, 2 x 2) computes the same numbers
    class Lay:
        y_stride, uv_stride, uv_step, u_offset, v_offset = 2, 1, 1, 4, 5
    n = len(Y)
    for j in (0, n // 3, n // 2, n - 1):
        buf = ref.pack(np.full((2, 2), Y[j], np.uint8), np.full((1, 1), U[j], np.uint8), np.full((1, 1), V[j], np.uint8), Lay, 6)
        assert (ref.to_bgr(buf, 2, 2, Lay) == fixed[j]).all()


def test_forward_conversion_round_trips():
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (8, 10, 3), dtype=np.uint8)
    bgr = np.repeat(np.repeat(bgr[::2, ::2], 2, 0), 2, 1)          # flat 2 x 2 blocks: chroma subsampling loses nothing
    class Lay:
        y_stride, uv_stride, uv_step, u_offset, v_offset = 10, 10, 2, 80, 81
    back = ref.to_bgr(ref.pack(*ref.from_bgr(bgr), Lay, 120), 10, 8, Lay)
    assert np.abs(back.astype(int) - bgr).max() <= 3
