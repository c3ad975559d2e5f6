"""The HIP kernels held to the float64 definitions of tests/f64_defs.py, through the matcher taps only (orb, pyramid_level,
small_image, page_small, last_candidates); the restatement in oracle/ is never the expected value here.  The GPU parity tests
say the kernels equal the restatement; these say that both equal the definition of each step:

(a)-(d) ORB (pyramid_kernel / resize kernels, blur_mark_kernel + the strip blur, fast_kernel, threshold_kernel's histogram
retainBest, the d_ictab centroid, describe_blurred_kernel for blur variant 0 and describe_kernel's per-sample integer blur for
variant 3) at 640x360, 1920x1080, the 2001x1125 page and one 3840x2160 frame with ORB-2000; (e) INTER_AREA of frames and pages
at the path's fractional factors; (f) the re-projection similarity of reproject_vt_kernel and reproject_kernel.  The bounds are
derived in f64_defs / f64_checks."""
import numpy as np
import pytest

import f64_checks as C
from conftest import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matchers(capi):
    ms = {b: capi.Matcher(capi.default_config(ocv_blur=b)) for b in (0, 3)}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def orb_inputs(synth):
    d = C.orb_inputs(synth)
    pages = synth.pages(2)
    d["synthetic_640x360"] = synth.frames(pages, 1, 640, 360, first=6)[0][0]
    d["natural_640x360"] = np.ascontiguousarray(d["natural_1080p"][200:560, 500:1140])
    d["synthetic_3840x2160"] = synth.frames(synth.pages(1), 1, 3840, 2160, first=5)[0][0]
    return d


@pytest.mark.parametrize("which,blur", [(w, b) for w in ("synthetic_640x360", "natural_640x360", "synthetic_1080p", "natural_1080p",
                                                          "page_2001x1125") for b in (0, 3)] + [("synthetic_3840x2160", 0)])
def test_orb_against_the_definitions(capi, oracle, matchers, orb_inputs, which, blur):
    img = orb_inputs[which]
    m = matchers[blur]
    kp, desc = m.orb(img)
    assert len(kp) >= (2000 if which == "synthetic_3840x2160" else 100)
    C.check_orb(img, m.cfg, blur, lambda l: m.pyramid_level(img, l, 0), lambda l: m.pyramid_level(img, l, 1), kp, desc,
                oracle.brief_pattern(m.cfg.patch_size))


@pytest.mark.parametrize("w,h", C.AREA_SHAPES)
def test_small_image_of_frames(matchers, synth, w, h):
    img = C.area_input(synth, w, h)
    C.check_area(matchers[0].small_image(img), img)
    noise = np.random.default_rng(w + h).integers(0, 256, img.shape, dtype=np.uint8)
    C.check_area(matchers[0].small_image(noise), noise)


def test_page_small_of_pages(capi, synth):
    pages = [C.golden_bgr("1-slide.png"), synth.pages(1)[0], synth.pages(1, 1600, 1200, seed=7)[0], synth.pages(1, 800, 450)[0],
             synth.pages(1, 1280, 720, seed=32)[0], synth.pages(1, 2600, 1462, seed=33)[0]]
    m = capi.Matcher(small_cfg(capi))
    m.add_pages(pages)
    m.finalize()
    for i, p in enumerate(pages):
        C.check_area(m.page_small(i), p)
    m.close()


def _deck_stats(capi, cfg, pages, frame_sets, st):
    m = capi.Matcher(cfg)
    m.add_pages(pages)
    m.finalize()
    smalls = [m.page_small(i) for i in range(len(pages))]
    shapes = [p.shape[:2] for p in pages]
    for frames in frame_sets:
        m.match_frames(frames)
        for i, fr in enumerate(frames):
            C.check_reprojection(fr, m.last_candidates(i), shapes, smalls, st)
    m.close()


@pytest.mark.parametrize("verify_model", [0, 1])
def test_reprojection_similarity_against_the_definition(capi, synth, cfg0_data, verify_model):
    """(f) the cfg0 deck and the mixed deck of test_gpu_parity.test_reprojection_through_both_kernels_and_the_frame_edges
    (800x450 and 1280x720 pages through reproject_vt_kernel, 2600x1462 through reproject_kernel, frames that ARE a page): every
    candidate with a similarity within similarity_bound of the definition, with the GPU's own page small images (8 frames per
    frame set, twice the parity test's, so that at least 20 candidates are checked).  Sharpness guard: at least 90 % of the
    candidates whose map is not collapsed (f64_checks.check_reprojection) have a bound below 1e-3."""
    st = {}
    pages, frames, _, _ = cfg0_data
    _deck_stats(capi, small_cfg(capi, verify_model=verify_model), list(pages), [frames], st)
    small = synth.pages(3, 800, 450, seed=31)
    mid = synth.pages(2, 1280, 720, seed=32)
    big = synth.pages(2, 2600, 1462, seed=33)
    fa, _, _ = synth.frames(small, 8, 640, 360, seed=41)
    fc = np.ascontiguousarray(mid[:, ::2, ::2])                          # the slide IS the frame
    fb, _, _ = synth.frames(big, 8, 1280, 720, seed=42)
    _deck_stats(capi, small_cfg(capi, verify_model=verify_model), list(small) + list(mid) + list(big),
                [np.concatenate([fa, fc]), fb], st)
    C.report("reprojection", **st)
    assert st["n"] >= 20 and st["sharp"] >= 0.9 * st["regular"], st
