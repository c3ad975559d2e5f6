"""The CPU restatement (oracle/) held to the float64 definitions of tests/f64_defs.py: ORB's pyramid, FAST, retainBest, the
intensity-centroid angle and rotated BRIEF, INTER_AREA at the path's fractional factors, the nearest-neighbour inverse warps
and the re-projection similarity.  The bounds are derived in f64_defs / f64_checks; this file validates them on the CPU before
tests/test_gpu_f64_definitions.py holds the HIP kernels to the same definitions."""
import numpy as np
import pytest

import f64_checks as C
import f64_defs as D
from conftest import small_cfg


@pytest.mark.parametrize("nf,sf,nl", [(2000, 1.2, 8), (500, 1.2, 8), (1000, 1.3, 5), (3, 1.5, 6)])
def test_orb_constants_equal_the_restatement(oracle, nf, sf, nl):
    cfg = oracle.default_config(nfeatures=nf, scale_factor=sf, nlevels=nl)
    for half in (31, 15, 8, 3):
        assert np.array_equal(D.umax(half), oracle.umax(half)), half
    assert np.array_equal(D.level_quotas(nf, cfg.scale_factor, nl), oracle.level_quotas(cfg))
    for w, h in ((1920, 1080), (2001, 1125), (3840, 2160), (640, 360), (317, 203)):
        ws, hs, sc = oracle.pyramid_sizes(w, h, cfg)
        dw, dh, ds = D.level_sizes(w, h, cfg.scale_factor, nl)
        assert np.array_equal(ws, dw) and np.array_equal(hs, dh) and np.array_equal(sc, ds), (w, h)


def test_fast_score_and_nms_equal_the_restatement(oracle, synth):
    pages = synth.pages(1)
    frames, _, _ = synth.frames(pages, 1, first=2)
    rng = np.random.default_rng(11)
    imgs = [oracle.gray(frames[0]), oracle.gray(C.golden_bgr("2-frame.png")), rng.integers(0, 256, (97, 131), dtype=np.uint8)]
    for t in (20, 5, 60):
        for g in imgs:
            s = D.fast_score(g, t)
            o = oracle.fast_score_map(g, t)
            assert np.array_equal(s[3:-3, 3:-3], o[3:-3, 3:-3]) and not o[:3].any() and not o[-3:].any()
            assert (s > 0).sum() > 100
            assert np.array_equal(np.where(D.fast_nms(s), s, 0), oracle.fast_nms_map(g, t))


@pytest.mark.parametrize("w,h", C.AREA_SHAPES)
def test_inter_area_at_the_path_factors(oracle, synth, w, h):
    """factors 4.165, 4.34, 8.33, 2.78, 1.39 and 4 (the integer fast path)."""
    img = C.area_input(synth, w, h)
    assert (img.shape[1], img.shape[0]) == (w, h)
    assert D.small_size(w, h) == oracle.small_size(w, h)
    C.check_area(oracle.small_image(img), img)
    rng = np.random.default_rng(w + h)                        # and pure noise: no flat areas whose means are integers
    noise = rng.integers(0, 256, img.shape, dtype=np.uint8)
    C.check_area(oracle.small_image(noise), noise)


def _similarity_M(rng, sw, sh, dw, dh, outside):
    s = rng.uniform(0.3, 2.5)
    a = rng.uniform(-np.pi, np.pi) if rng.random() < 0.5 else rng.uniform(-0.2, 0.2)
    c, si = s * np.cos(a), s * np.sin(a)
    cx, cy = (sw / 2, sh / 2) if not outside else (rng.uniform(0, sw), rng.uniform(0, sh))
    tx, ty = cx - (c * dw / 2 - si * dh / 2), cy - (si * dw / 2 + c * dh / 2)
    return np.array([c, -si, tx, si, c, ty])


def _homography(rng, sw, sh, dw, dh):
    A = _similarity_M(rng, sw, sh, dw, dh, rng.random() < 0.3)
    H = np.array([[A[0], A[1], A[2]], [A[3], A[4], A[5]], [0.0, 0.0, 1.0]])
    H[2, 0] = rng.uniform(-0.3, 0.3) / dw                    # keystone; the denominator stays within [0.4, 1.6] on the page
    H[2, 1] = rng.uniform(-0.3, 0.3) / dh
    H[:2] += rng.normal(0, 0.02, (2, 3)) * np.array([1, 1, 10])
    return H


def test_nearest_warps_equal_the_definition(oracle, synth):
    """warp_affine_nn (10-bit fixed point) and warp_perspective_nn equal warp_nearest on every non-ambiguous pixel, for random
    similarities, similarities that map part of the page outside the frame, and random homographies."""
    frame = C.golden_bgr("2-frame.png")
    sh, sw = frame.shape[:2]
    rng = np.random.default_rng(3)
    amb_total = n_total = outside_seen = 0
    for i in range(12):
        dw, dh = [(800, 450), (1280, 720), (2001, 1125)][i % 3]
        M = _similarity_M(rng, sw, sh, dw, dh, outside=i % 2 == 1)
        want, amb = D.warp_nearest(frame, M, dw, dh)
        got = oracle.warp_affine_nn(frame, M, dw, dh)
        assert not (got != want).any(axis=2)[~amb].any(), i
        amb_total += int(amb.sum()); n_total += amb.size
        outside_seen += int((want == 0).all(axis=2).mean() > 0.05)
        H = _homography(rng, sw, sh, dw, dh)
        want, amb = D.warp_nearest(frame, H, dw, dh)
        got = oracle.warp_perspective_nn(frame, H, dw, dh)
        assert not (got != want).any(axis=2)[~amb].any(), i
        amb_total += int(amb.sum()); n_total += amb.size
    assert outside_seen >= 3
    assert amb_total / n_total < 0.02
    C.report("warp", ambiguous_frac=amb_total / n_total)


@pytest.fixture(scope="module")
def orb_inputs(synth):
    return C.orb_inputs(synth)


@pytest.mark.parametrize("blur", [0, 3])
@pytest.mark.parametrize("which", ["synthetic_1080p", "page_2001x1125", "natural_1080p"])
def test_orb_against_the_definitions(oracle, orb_inputs, which, blur):
    """(a)-(d) of f64_checks on oracle.orb / oracle.pyramid_level with the ORB defaults."""
    img = orb_inputs[which]
    cfg = oracle.default_config(ocv_blur=blur)
    kp, desc = oracle.orb(img, cfg)
    C.check_orb(img, cfg, blur, lambda l: oracle.pyramid_level(img, cfg, l, 0), lambda l: oracle.pyramid_level(img, cfg, l, 1),
                kp, desc, oracle.brief_pattern(cfg.patch_size))


@pytest.mark.parametrize("verify_model", [0, 1])
def test_reprojection_similarity_against_the_definition(oracle, cfg0_data, verify_model):
    """(f) on the restatement's trace of the cfg0 deck: every re-projected candidate's similarity within similarity_bound of the
    definition, with the restatement's own page small images."""
    pages, frames, _, _ = cfg0_data
    db = oracle.PageDB(small_cfg(oracle, verify_model=verify_model))
    for p in pages:
        db.add_page(p)
    assert db.finalize() == 0
    smalls = [oracle.small_image(p) for p in pages]
    shapes = [p.shape[:2] for p in pages]
    st = {}
    for fr in frames:
        _, cands = db.match_frame_trace(fr)
        C.check_reprojection(fr, cands, shapes, smalls, st)
    assert st["n"] >= 5 and st["sharp"] >= 0.9 * st["regular"], st
    C.report("reprojection", **st)
