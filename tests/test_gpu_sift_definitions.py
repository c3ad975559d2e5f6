"""The HIP SIFT kernels (csrc/sift.hip.h) held to the float64 definitions of tests/f64_defs_sift.py, through Matcher.sift,
Matcher.sift_layer and the gray tap (pyramid_level 0) only; the restatement in oracle/ is never the expected value of a
definition check here.  tests/test_gpu_sift.py says the kernels equal the restatement; these say that the kernels equal the
definition of each step — sift_base_kernel and the blur kernels (check_sift_pyramid), sift_half_kernel (the octave step),
sift_extrema_kernel and sift_refine_kernel (check_sift_keypoints, check_sift_orientation), sift_select_kernel
(check_sift_selection) and sift_describe_kernel (check_sift_descriptors) — within the bounds derived in f64_checks.

The sweep runs the pyramid check at sigmas that take every unrolled instance of the stream blur (7 to 27 taps) and the generic
tile kernel (small top octaves; 29, 33 and 39 taps) on images at the kernels' size switches; there, and only there, the layers
are also compared bit for bit with the restatement."""
import numpy as np
import pytest

import f64_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m(capi):
    mm = capi.Matcher(capi.default_config())
    yield mm
    mm.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sift_against_the_definitions(capi, m, name):
    img, sigma = C.sift_inputs()[name]
    sc = lambda n=0: capi.sift_config(sigma=sigma, nfeatures=n)
    G, DOG, kp, desc, points = C.check_sift(img, m.pyramid_level(img, 0, 0), sigma, lambda n: m.sift(img, sc(n)),
                                            lambda o, i, dog: m.sift_layer(img, o, i, dog, sc()), None, name)
    assert len(kp) >= 30 and len(points) >= 20


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sift_selection(capi, m, name):
    img, sigma = C.sift_inputs()[name]
    C.check_sift_selection(lambda n: m.sift(img, capi.sift_config(sigma=sigma, nfeatures=n)), (1, 37), name)


def test_sweep_covers_every_blur_instance():
    unrolled, generic = C.sift_sweep_taps()
    assert set(range(7, 28, 2)) <= unrolled and {29, 33, 39} <= generic, (sorted(unrolled), sorted(generic))


@pytest.mark.parametrize("sigma", C.SIFT_SWEEP_SIGMAS)
@pytest.mark.parametrize("name", ["33x40", "16x17", "131x97"])
def test_sift_pyramid_sweep(capi, oracle, m, name, sigma):
    img = C.sift_sweep_images()[name]
    sc, osc = capi.sift_config(sigma=sigma), oracle.sift_config(sigma=sigma)
    G, DOG = C.check_sift_pyramid(m.pyramid_level(img, 0, 0), sigma, lambda o, i, dog: m.sift_layer(img, o, i, dog, sc), None,
                                  "%s@%g" % (name, sigma))
    for o in range(len(G)):                                     # and the parity with the restatement on these kernel paths
        for i in range(len(G[o])):
            assert np.array_equal(G[o][i], oracle.sift_layer(img, o, i, False, osc)), (o, i)
        for i in range(len(DOG[o])):
            assert np.array_equal(DOG[o][i], oracle.sift_layer(img, o, i, True, osc)), (o, i)
