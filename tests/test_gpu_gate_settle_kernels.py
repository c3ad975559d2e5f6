"""The kernels of the gate reference ANCHOR, with and without a gate settle, on their own (include/slideo_amd.h "Gate reference",
"Gate settle"; plain ANCHOR is the settle with a cap of 0 and no previous frame), every comparison exact equality.

slideo_small_carried_ssd — gate_carried_ssd_kernel — against numpy: n = 1, 2 and 65 images (the grid's second dimension is n + 1 and
the host cuts a pair across fewer blocks as n grows) of L = 3 sw sh = 105 (one block, a body of 25 dwords), 2139 (several blocks
of one dword per thread, a ragged tail) and 358 197 bytes (the small image of a 640x360 frame).  The tap uploads the anchor, the
previous frame and the images back to back, so with these odd lengths they start at every byte alignment.  Contents: random bytes,
and all-0 against all-255, the largest SSD.  use_valid: the validity map of a 640x360 mask with a hole (461x259).  Without a
previous frame (None: plain ANCHOR's launch) the grid has n rows and the host cuts a pair by n, not n + 1: the same shapes — one
block; several blocks with a ragged tail; the workload's size —, the first n values of the same numpy.

slideo_gate_settle_walk — gate_settle_kernel — against the restatement's integer walk (tests/gate_settle_ref.py): random integer
vectors of 8 components give the table of dot products and the norms exactly; n = 1, 63, 64, 65, 130 around the 64-lane window;
max_defer = 0, 1, 3, 70 (a run of deferred frames that crosses the window and reaches its cap behind it) and 2**30; the carried
count zero and nonzero; the state "none".  thr_c is a quantile of the SSDs that occur, thr_s separates the walk's small steps from its
large ones, and the test asserts on the
restatement, before anything is compared, that every branch occurs: unchanged, matched-still, matched-by-cap, deferred.
A cap of 0 — where the kernel reads neither the carried count nor any previous-frame SSD — is held to the plain anchor rule written
as its own loop here, not to the settle's restatement."""
import numpy as np
import pytest

import gate_mask_ref as gref
import gate_settle_ref as sref
from conftest import small_cfg

pytestmark = pytest.mark.gpu

SIZES = [(5, 7), (23, 31), (461, 259)]
NS = [1, 2, 65]
W, H = 640, 360


@pytest.fixture(scope="module")
def plain(capi):
    m = capi.Matcher(small_cfg(capi))                            # the taps need no pages
    yield m
    m.close()


@pytest.fixture(scope="module")
def masked(capi, oracle):
    mask = np.full((H, W), 255, np.uint8)
    mask[190:350, 390:630] = 0
    m = capi.Matcher(small_cfg(capi))
    m.set_frame_mask_scope(capi.MASK_DETECT | capi.MASK_GATE)
    m.set_frame_mask(mask)
    valid, nv = gref.validity_map(oracle, mask)
    assert valid.shape == (259, 461) and 0 < nv < valid.size
    yield m, valid
    m.close()


def _ssd(a, b, valid=None):
    d = a.astype(np.int64) - b.astype(np.int64)
    d = (d * d).sum(axis=-1)
    return int(d.sum() if valid is None else d[valid].sum())


def _want(anchor, prev, s, valid=None):
    return np.array([_ssd(anchor, x, valid) for x in s] + [_ssd(prev, s[0], valid)], np.uint64)


def _random(n, sw, sh):
    rng = np.random.default_rng(1000 * sw + n)
    return rng.integers(0, 256, (n + 2, sh, sw, 3), dtype=np.uint8)


@pytest.mark.parametrize("sw,sh", SIZES)
@pytest.mark.parametrize("n", NS)
def test_carried_ssd_random_bytes(plain, n, sw, sh):
    x = _random(n, sw, sh)
    got = plain.small_carried_ssd(x[0], x[1], x[2:])
    assert got.dtype == np.uint64 and np.array_equal(got, _want(x[0], x[1], x[2:]))


@pytest.mark.parametrize("sw,sh", SIZES)
@pytest.mark.parametrize("n", NS)
def test_carried_ssd_largest(plain, n, sw, sh):
    """The anchor all 0 against images that are all 255 (every second one, the others all 0), the previous frame all 255 against
    image 0: 255^2 per byte over the whole pair."""
    anchor = np.zeros((sh, sw, 3), np.uint8)
    prev = np.full((sh, sw, 3), 255, np.uint8)
    s = np.zeros((n, sh, sw, 3), np.uint8)
    s[1::2] = 255
    top = 255 * 255 * 3 * sw * sh
    want = np.array([top if i % 2 else 0 for i in range(n)] + [top], np.uint64)
    assert np.array_equal(_want(anchor, prev, s), want)
    assert np.array_equal(plain.small_carried_ssd(anchor, prev, s), want)
    want = np.array([0 if i % 2 else top for i in range(n)] + [0], np.uint64)
    assert np.array_equal(plain.small_carried_ssd(prev, anchor, s), want)


def test_carried_ssd_under_a_validity_map(masked):
    m, valid = masked
    x = _random(3, 461, 259)
    want = _want(x[0], x[1], x[2:], valid)
    assert not np.array_equal(want, _want(x[0], x[1], x[2:])), "the hole matters"
    assert np.array_equal(m.small_carried_ssd(x[0], x[1], x[2:], use_valid=True), want)
    assert np.array_equal(m.small_carried_ssd(x[0], x[1], x[2:]), _want(x[0], x[1], x[2:])), "whole images: the map is not in the way"
    x[2:] = 255
    x[0] = 0
    assert m.small_carried_ssd(x[0], x[1], x[2:], use_valid=True)[0] == 255 * 255 * 3 * int(valid.sum())


NO_PREV = [(n, sw, sh) for sw, sh in SIZES[:2] for n in NS] + [(2,) + SIZES[2]]


@pytest.mark.parametrize("n,sw,sh", NO_PREV)
def test_carried_ssd_without_a_previous_frame(plain, n, sw, sh):
    x = _random(n, sw, sh)
    got = plain.small_carried_ssd(x[0], None, x[2:])
    assert got.dtype == np.uint64 and got.shape == (n,) and np.array_equal(got, _want(x[0], x[1], x[2:])[:n])
    anchor = np.zeros((sh, sw, 3), np.uint8)
    s = np.zeros((n, sh, sw, 3), np.uint8)
    s[::2] = 255
    want = _want(anchor, anchor, s)[:n]
    assert want[0] == 255 * 255 * 3 * sw * sh and np.array_equal(plain.small_carried_ssd(anchor, None, s), want)


def test_carried_ssd_without_a_previous_frame_under_a_validity_map(masked):
    m, valid = masked
    x = _random(2, 461, 259)
    want = _want(x[0], x[1], x[2:], valid)[:2]
    assert not np.array_equal(want, _want(x[0], x[1], x[2:])[:2]), "the hole matters"
    assert np.array_equal(m.small_carried_ssd(x[0], None, x[2:], use_valid=True), want)


def test_carried_ssd_refusals(capi, plain, masked):
    m, _ = masked
    x = _random(2, 5, 7)
    with pytest.raises(capi.SlideoError) as e:
        m.small_carried_ssd(x[0], x[1], x[2:], use_valid=True)
    assert e.value.code == 1, "another size than the map's"
    with pytest.raises(capi.SlideoError) as e:
        plain.small_carried_ssd(x[0], x[1], x[2:], use_valid=True)
    assert e.value.code == 4, "no validity map in force"
    big = np.zeros((3, 400, 400, 3), np.uint8)
    with pytest.raises(capi.SlideoError) as e:
        plain.small_carried_ssd(big[0], big[1], big[2:])
    assert e.value.code == 1, "beyond small_area"


# ---- the walk -----------------------------------------------------------------------------------------------------------------------------
WALK_NS = [1, 63, 64, 65, 130]
MAX_DEFERS = [0, 1, 3, 70, 2 ** 30]


def _walk_case(n, max_defer, none, d_in, seed):
    """Frames as integer vectors of 8 components: a random walk of small steps (still, drifting away from the anchor) and large
    steps (away, not still) with returns to the start (not away); every third case is large steps almost throughout and never
    returns, so that runs of deferred frames grow past a window and reach a cap of 70."""
    rng = np.random.default_rng(seed)
    style = (seed // 3 + seed) % 3
    step = np.where(rng.random((n, 1)) < (0.25, 0.6, 0.995)[style], rng.integers(-40, 41, (n, 8)), rng.integers(-2, 3, (n, 8)))
    x = 1000 + np.cumsum(step, axis=0)
    if n > 8 and style != 2:
        x[rng.integers(1, n, n // 8)] = x[0]
    # the carried anchor: frame 0's neighbour, or, where a count is carried in, far from it (frame 0 is away and continues the run)
    anchor, prev = x[0] + (200 if d_in else rng.integers(-3, 4, 8)), x[0] + rng.integers(-30, 31, 8)
    dot = (x @ x.T).astype(np.int64)
    norm = (x * x).sum(axis=1).astype(np.int64)
    table = norm[:, None] + norm[None, :] - 2 * dot
    carried = np.array([((anchor - v) ** 2).sum() for v in x] + [((prev - x[0]) ** 2).sum()], np.int64)
    thr_s = 8 * 2 * 2 + 1                                        # the small steps are still (at most 2 per component), the large ones hardly ever
    thr_c = int(np.quantile(np.concatenate([carried[:n], table[np.triu_indices(n, 1)]]), (0.3, 0.3, 0.02)[style])) + 1
    return dot, norm, table, carried, thr_c, thr_s


def _walk_cases():
    out = []
    for n in WALK_NS:
        for max_defer in MAX_DEFERS:
            for none, d_in in ((False, 0), (False, min(max_defer, 5)), (True, 0)):
                out.append((n, max_defer, none, d_in))
    return out


def test_the_walk_cases_take_every_branch():
    kinds, crossing, late_cap, carried_d = [], False, False, False
    for k, (n, max_defer, none, d_in) in enumerate(_walk_cases()):
        dot, norm, table, carried, thr_c, thr_s = _walk_case(n, max_defer, none, d_in, k)
        fl, ssd, kind, last, d_out = sref.walk(table, carried, thr_c, thr_s, max_defer, d_in, none)
        kinds.append(kind)
        i = 1 if none else 0                                     # the kernel's windows: 64 frames from behind the last matched frame
        while i < n:
            hit = np.nonzero(fl[i:i + 64])[0]
            if len(hit):
                i += int(hit[0]) + 1
                continue
            crossing |= i + 64 < n and kind[i + 63] == sref.DEFERRED
            i += 64
        late_cap |= max_defer == 70 and bool((kind[64:] == sref.MATCHED_CAP).any())
        carried_d |= d_in > 0 and len(kind) > 0 and kind[0] in (sref.DEFERRED, sref.MATCHED_CAP)
    kinds = np.concatenate(kinds)
    for kd in (sref.UNCHANGED, sref.DEFERRED, sref.MATCHED_STILL, sref.MATCHED_CAP):
        assert (kinds == kd).sum() >= 10, kd
    assert crossing and late_cap and carried_d


@pytest.mark.parametrize("n", WALK_NS)
def test_walk(plain, n):
    for k, (cn, max_defer, none, d_in) in enumerate(_walk_cases()):
        if cn != n:
            continue
        dot, norm, table, carried, thr_c, thr_s = _walk_case(n, max_defer, none, d_in, k)
        fl, ssd, kind, last, d_out = sref.walk(table, carried, thr_c, thr_s, max_defer, d_in, none)
        got = plain.gate_settle_walk(dot, norm, carried, thr_c, thr_s, max_defer, d_in, none)
        what = (n, max_defer, none, d_in)
        assert np.array_equal(got[0], fl), (what, "flags", np.nonzero(got[0] != fl)[0][:8])
        assert np.array_equal(got[1].astype(np.int64), ssd), (what, "SSDs")
        assert got[2] == last and got[3] == d_out, (what, got[2:], last, d_out)


def test_walk_all_deferred_and_all_matched(plain):
    """The two extremes over three windows: nothing is ever still and the cap is never reached (every frame deferred, the count
    carried from window to window), and a cap of 0 (every away frame matched: the ANCHOR rule)."""
    n = 130
    dot, norm, table, carried, _, _ = _walk_case(n, 0, False, 0, 99)
    fl, ssd, kind, last, d_out = sref.walk(table, carried, 0, 0, 2 ** 30, 7, False)
    assert (kind == sref.DEFERRED).all() and last == -1 and d_out == n + 7
    got = plain.gate_settle_walk(dot, norm, carried, 0, 0, 2 ** 30, 7, False)
    assert not got[0].any() and np.array_equal(got[1].astype(np.int64), ssd) and got[2:] == (-1, n + 7)
    got = plain.gate_settle_walk(dot, norm, carried, 0, 0, 100, 7, False)
    fl, ssd, kind, last, d_out = sref.walk(table, carried, 0, 0, 100, 7, False)
    assert kind[93] == sref.MATCHED_CAP and np.array_equal(got[0], fl) and got[2:] == (last, d_out)
    fl, ssd, kind, last, d_out = sref.walk(table, carried, 0, 0, 0, 0, False)
    assert fl.all() and last == n - 1
    got = plain.gate_settle_walk(dot, norm, carried, 0, 0, 0, 0, False)
    assert got[0].all() and np.array_equal(got[1].astype(np.int64), ssd) and got[2:] == (n - 1, 0)


def _anchor_rule(table, carried, thr, none):
    """Plain ANCHOR, frame by frame: the carried anchor until a frame is flagged, then the last flagged frame."""
    n = len(table)
    flags, ssd, a = np.zeros(n, np.uint8), np.zeros(n, np.int64), -1
    for j in range(n):
        if none and j == 0:
            flags[0], a = 1, 0
            continue
        ssd[j] = carried[j] if a < 0 else table[a, j]
        if ssd[j] >= thr:
            flags[j], a = 1, j
    return flags, ssd, a


def test_a_cap_of_0_is_the_plain_anchor_rule(plain):
    cases, flagged, unflagged, carried_across = [], 0, 0, False
    for k, n in enumerate(WALK_NS):
        for none in (False, True):
            dot, norm, table, carried, thr_c, thr_s = _walk_case(n, 0, none, 0, 300 + 2 * k + none)
            cases.append((n, none, dot, norm, table, carried, thr_c, thr_s))
    # nothing flagged over a whole window behind the carried anchor: the walk moves on by 64 frames with the anchor still -1
    dot, norm, table, carried, _, thr_s = _walk_case(130, 0, False, 0, 77)
    cases.append((130, False, dot, norm, table, carried, int(carried[:100].max()) + 1, thr_s))
    want = []
    for n, none, dot, norm, table, carried, thr_c, thr_s in cases:
        fl, ssd, last = _anchor_rule(table, carried, thr_c, none)
        want.append((fl, ssd, last))
        flagged += int(fl.sum()) - int(none)
        unflagged += int((fl == 0).sum())
        carried_across |= not none and n > 64 and not fl[:64].any()
    assert flagged >= 10 and unflagged >= 10 and carried_across
    for (n, none, dot, norm, table, carried, thr_c, thr_s), (fl, ssd, last) in zip(cases, want):
        got = plain.gate_settle_walk(dot, norm, carried, thr_c, thr_s, 0, 0, none)
        assert np.array_equal(got[0], fl), (n, none, "flags", np.nonzero(got[0] != fl)[0][:8])
        assert np.array_equal(got[1].astype(np.int64), ssd), (n, none, "SSDs")
        assert got[2:] == (last, 0), (n, none, got[2:], last)
    # `still` is not consulted: any thr_s gives the same output
    n, none, dot, norm, table, carried, thr_c, _ = cases[-2]
    fl, ssd, last = want[-2]
    for thr_s in (0, 2 ** 62):
        got = plain.gate_settle_walk(dot, norm, carried, thr_c, thr_s, 0, 0, none)
        assert np.array_equal(got[0], fl) and np.array_equal(got[1].astype(np.int64), ssd) and got[2:] == (last, 0), thr_s


def test_walk_refusals(capi, plain):
    dot, norm, table, carried, thr_c, thr_s = _walk_case(4, 3, False, 0, 5)
    for max_defer, d_in in ((-1, 0), (3, 4), (3, -1)):
        with pytest.raises(capi.SlideoError) as e:
            plain.gate_settle_walk(dot, norm, carried, thr_c, thr_s, max_defer, d_in, False)
        assert e.value.code == 1
