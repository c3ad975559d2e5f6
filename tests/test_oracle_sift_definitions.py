"""The CPU restatement of SIFT (oracle/sift_oracle.h) held to the float64 definitions of tests/f64_defs_sift.py, step by step on
its own upstream outputs (f64_checks.check_sift_*): pyramid, raw extrema, refinement, orientation, selection, descriptor.  The
bounds are derived in f64_checks; this file validates them on the CPU before tests/test_gpu_sift_definitions.py holds the HIP
kernels to the same definitions, and its sensitivity tests show that each check catches a small, deliberate error."""
import numpy as np
import pytest

import f64_checks as C
import f64_defs_sift as S

_CACHE = {}


def _run(oracle, name):
    """The checked restatement outputs of an input, computed once: (G, DOG, kp, desc, points)."""
    if name not in _CACHE:
        img, sigma = C.sift_inputs()[name]
        sc = lambda n=0: oracle.sift_config(sigma=sigma, nfeatures=n)
        _, _, st = oracle.sift(img, sc())
        _CACHE[name] = C.check_sift(img, oracle.gray(img), sigma, lambda n: oracle.sift(img, sc(n))[:2],
                                    lambda o, i, dog: oracle.sift_layer(img, o, i, dog, sc()), st, name)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sift_against_the_definitions(oracle, name):
    G, DOG, kp, desc, points = _run(oracle, name)
    assert len(kp) >= 30 and len(points) >= 20


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_solve_constant_is_the_definitions_own_f32_error(oracle, name):
    """SOLVE_K: the definition in np.float32 against the definition in float64."""
    _, DOG, _, _, _ = _run(oracle, name)
    k = C.sift_solve_constant(DOG, C.sift_inputs()[name][1])
    C.report("sift-solve", image=name, f32_minus_f64=float(k), constant=C.SOLVE_K)
    assert 0 < k <= C.SOLVE_K


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_sift_selection(oracle, name):
    img, sigma = C.sift_inputs()[name]
    C.check_sift_selection(lambda n: oracle.sift(img, oracle.sift_config(sigma=sigma, nfeatures=n))[:2], (1, 37), name)


def test_sweep_covers_every_blur_instance():
    unrolled, generic = C.sift_sweep_taps()
    assert set(range(7, 28, 2)) <= unrolled and {29, 33, 39} <= generic, (sorted(unrolled), sorted(generic))
    assert all(0.5 < s <= 2.4 for s in C.SIFT_SWEEP_SIGMAS)
    assert 25 in {n for _, _, n, _, _ in S.blur_plan(277, 189, C.sift_inputs()["C"][1])}      # input C runs the 25-tap instance too


@pytest.mark.parametrize("sigma", C.SIFT_SWEEP_SIGMAS)
@pytest.mark.parametrize("name", ["33x40", "16x17", "131x97"])
def test_sift_pyramid_sweep(oracle, name, sigma):
    img = C.sift_sweep_images()[name]
    sc = oracle.sift_config(sigma=sigma)
    C.check_sift_pyramid(oracle.gray(img), sigma, lambda o, i, dog: oracle.sift_layer(img, o, i, dog, sc), oracle.sift(img, sc)[2]["octaves"],
                         "%s@%g" % (name, sigma))


# ---- sensitivity: each check raises on a small, deliberate error (input B: 25 refined points, all decided) --------------------

@pytest.fixture(scope="module")
def b(oracle):
    img, sigma = C.sift_inputs()["B"]
    G, DOG, kp, desc, points = _run(oracle, "B")
    return dict(img=img, sigma=sigma, gray=oracle.gray(img), G=G, DOG=DOG, kp=kp, desc=desc, points=points)


def _layers(b, swap):
    def layer(o, i, dog):
        if not dog and (o, i) in swap:
            return swap[(o, i)]
        return b["DOG"][o][i] if dog else b["G"][o][i]
    return layer


def test_the_unchanged_outputs_pass_from_the_cache(b):
    C.check_sift_pyramid(b["gray"], b["sigma"], _layers(b, {}))
    points = C.check_sift_keypoints(b["DOG"], b["kp"], b["sigma"])
    C.check_sift_orientation(b["G"], b["kp"], points)
    C.check_sift_descriptors(b["G"], b["kp"], b["desc"])


def test_a_layer_blurred_with_2_percent_more_sigma_is_caught(b):
    wrong = S.blur(b["G"][0][1], S.layer_sigmas(b["sigma"])[1] * 1.02).astype(np.float32)
    with pytest.raises(AssertionError, match="blur"):
        C.check_sift_pyramid(b["gray"], b["sigma"], _layers(b, {(0, 2): wrong}))
    base = S.blur(S.upsample2(b["gray"]), S.base_sigma(b["sigma"]) * 1.02).astype(np.float32)
    with pytest.raises(AssertionError, match="base"):
        C.check_sift_pyramid(b["gray"], b["sigma"], _layers(b, {(0, 0): base}))


def test_a_layer_shifted_by_one_pixel_is_caught(b):
    for axis in (0, 1):
        with pytest.raises(AssertionError, match="blur"):
            C.check_sift_pyramid(b["gray"], b["sigma"], _layers(b, {(1, 2): np.roll(b["G"][1][2], 1, axis=axis)}))


@pytest.mark.parametrize("field", ["x", "y"])
def test_a_keypoint_moved_by_a_hundredth_of_a_pixel_is_caught(b, field):
    kp = b["kp"].copy()
    kp[field][kp[field] == kp[field][0]] += np.float32(0.01)
    with pytest.raises(AssertionError, match="no refined candidate"):
        C.check_sift_keypoints(b["DOG"], kp, b["sigma"])


def test_a_size_off_by_a_thousandth_is_caught(b):
    kp = b["kp"].copy()
    kp["size"] *= np.float32(1.001)
    with pytest.raises(AssertionError, match="size"):
        C.check_sift_keypoints(b["DOG"], kp, b["sigma"])


def test_a_response_off_by_a_thousandth_and_a_wrong_xi_byte_are_caught(b):
    kp = b["kp"].copy()
    kp["response"] *= np.float32(1.001)
    with pytest.raises(AssertionError, match="response"):
        C.check_sift_keypoints(b["DOG"], kp, b["sigma"])
    kp = b["kp"].copy()
    kp["octave"] += 2 << 16
    with pytest.raises(AssertionError, match="octave"):
        C.check_sift_keypoints(b["DOG"], kp, b["sigma"])


def test_an_angle_off_by_two_degrees_is_caught(b):
    kp = b["kp"].copy()
    kp["angle"] = (kp["angle"] + np.float32(2.0)) % np.float32(360.0)
    with pytest.raises(AssertionError, match="deg"):
        C.check_sift_orientation(b["G"], kp, b["points"])


def test_descriptor_orientation_bins_rolled_by_one_are_caught(b):
    desc = np.ascontiguousarray(np.roll(b["desc"].reshape(-1, 16, 8), 1, axis=2).reshape(-1, 128))
    with pytest.raises(AssertionError, match="descriptor of keypoint"):
        C.check_sift_descriptors(b["G"], b["kp"], desc)


def test_a_descriptor_cell_scaled_by_5_percent_is_caught(b):
    desc = b["desc"].copy().reshape(-1, 16, 8)
    assert desc[0, 5].max() >= 30
    desc[:, 5] = np.minimum(np.rint(desc[:, 5] * 1.05), 255).astype(np.uint8)
    with pytest.raises(AssertionError, match="descriptor of keypoint"):
        C.check_sift_descriptors(b["G"], b["kp"], desc.reshape(-1, 128))


def test_a_dropped_decided_keypoint_is_caught(b):
    kp = b["kp"]
    keep = kp["x"] != kp["x"][len(kp) // 2]
    assert 0 < (~keep).sum() < 4
    with pytest.raises(AssertionError, match="missing"):
        C.check_sift_keypoints(b["DOG"], kp[keep], b["sigma"])


def test_an_added_spurious_keypoint_is_caught(b):
    extra = b["kp"][:1].copy()
    extra["x"] += 3; extra["y"] += 2
    with pytest.raises(AssertionError, match="no refined candidate"):
        C.check_sift_keypoints(b["DOG"], np.concatenate([b["kp"], extra]), b["sigma"])
    angle = b["kp"][:1].copy()
    angle["angle"] = (angle["angle"] + 95) % 360
    with pytest.raises(AssertionError, match="is no peak"):
        C.check_sift_orientation(b["G"], np.concatenate([b["kp"], angle]), [p[:5] + (p[5] + ([len(b["kp"])] if 0 in p[5] else []),) for p in b["points"]])
