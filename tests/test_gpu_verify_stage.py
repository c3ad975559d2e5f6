"""The verify stage's kernels — vote_kernel, ransac_kernel, ransac_h_kernel with its tail and the refine kernels, rate_kernel,
verdict_kernel — against their definition (tests/verify_ref.py) on constructed features (tests/verify_cases.py), driven through the
frame-features tap Matcher.match_features: candidates, votes, inliers, survivors and verdicts exactly, transforms at the project's
bar (rtol 1e-5, atol 1e-6 * [1, 1, 1e3, 1, 1, 1e3, 1e-3, 1e-3, 1], NaN equal to NaN) for EVERY candidate — no excuse for
ill-conditioned ones —, the similarities the verdict rule reads are the GPU's own, each held to the float64 re-projection bound."""
import numpy as np
import pytest

import f64_checks as C
import verify_cases as VC
import verify_ref as R
from conftest import small_cfg

pytestmark = pytest.mark.gpu

CASES = VC.all_cases()
SCALE = np.array([1, 1, 1e3, 1, 1, 1e3, 1e-3, 1e-3, 1])
ENGINES = ("mfma2", "mfma4", "valu")


def _matcher(capi, case, cfg):
    m = capi.Matcher(cfg)
    smalls = {}
    for p in case.pages:
        if p.img not in smalls:
            smalls[p.img] = m.small_image(VC.page_image(p.img))
        m.add_page_features(VC.PAGE_W, VC.PAGE_H, VC.keypoints(p.xy), p.desc, smalls[p.img])
    m.finalize()
    return m, smalls


def _inputs(case):
    if getattr(case, "_inputs", None) is None:
        n = len(case.frames)
        frames = np.stack([case.frame_pixels(i) for i in range(n)])
        case._inputs = (frames, [VC.keypoints(f.xy) for f in case.frames], [f.desc for f in case.frames])
    return case._inputs


def _run(m, case):
    frames, kps, descs = _inputs(case)
    v = m.match_features(frames, kps, descs)
    return v, [m.last_candidates(i) for i in range(len(frames))]


def _same_records(a, b):
    (va, ca), (vb, cb) = a, b
    return va.tobytes() == vb.tobytes() and len(ca) == len(cb) and all(x.tobytes() == y.tobytes() for x, y in zip(ca, cb))


@pytest.mark.parametrize("fa", CASES, ids=VC.case_id)
def test_kernels_equal_definition(capi, oracle, monkeypatch, fa):
    """Planted-model recovery (R2, R3, H1): the inlier COUNT equals the planted set's (the records carry no mask; the restatement's
    mask is held to the planted set itself in test_oracle_verify_stage) and the model's residual over the exact planted inliers is
    at most 4 x the restatement estimator's own, measured in the same run (3e-5 .. 1e-4 px, R3: 0.5 / 0.25 px under the band's pull:
    test_oracle_verify_stage's docstring)."""
    case = VC.build(*fa)
    cfg = small_cfg(capi, **case.cfg)
    ocfg = small_cfg(oracle, **case.cfg)
    ref = VC.reference(case, oracle, ocfg)
    m, smalls = _matcher(capi, case, cfg)
    runs = []
    for env in case.envs:
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        runs.append(_run(m, case))
    for r in runs[1:]:
        assert _same_records(runs[0], r), "%s: the records differ between %s" % (case.name, case.envs)
    v, cands = runs[0]
    m.close()
    frames = _inputs(case)[0]
    ofs = np.concatenate([[0], np.cumsum([len(p.xy) for p in case.pages])])
    shapes = [(VC.PAGE_H, VC.PAGE_W)] * len(case.pages)
    page_small = [smalls[p.img] for p in case.pages]
    stats = {}
    for fi, f in enumerate(case.frames):
        gv, gc, st = v[fi], cands[fi], ref[fi]
        assert list(gc["page_idx"]) == [c.page for c in st.cands], case.name
        assert list(gc["n_votes"]) == [c.n_votes for c in st.cands]
        assert list(gc["inliers"]) == [c.inliers for c in st.cands]
        assert list(gc["survived"]) == [int(i in st.surv) for i in range(len(st.cands))]
        for a, c in zip(gc, st.cands):
            print("%s frame %d page %d: %d votes %d inliers, max |dM| %.3g" %
                  (case.name, fi, c.page, c.n_votes, c.inliers, float(np.nan_to_num(np.abs(a["transform"] - c.M.reshape(9))).max())))
            assert np.allclose(a["transform"], c.M.reshape(9), rtol=1e-5, atol=1e-6 * SCALE, equal_nan=True), (case.name, c.page)
        sims = {i: gc["similarity"][i] for i in st.surv}
        page, sim, inl, nk = R.verdict(cfg, st, sims)
        assert (gv["page_idx"], gv["inliers"], gv["n_keypoints"]) == (page, inl, nk), case.name
        assert gv["similarity"] == sim
        VC.check_expectations(case, fi, list(gc["page_idx"]), list(gc["n_votes"]), list(gc["inliers"]), list(gc["survived"]),
                              int(gv["page_idx"]))
        if case.expect.get("identical_frames") and 0 < fi < 64:
            assert gv.tobytes() == v[0].tobytes() and gc.tobytes() == cands[0].tobytes()        # the same features, the same frame
        else:
            C.check_reprojection(frames[fi], gc, shapes, page_small, stats)
        if "planted" in case.expect:
            for a, c in zip(gc, st.cands):
                if c.n_votes < 200:
                    continue
                qs = [q for q, _ in c.votes]; ts = [t - ofs[c.page] for _, t in c.votes]
                own = VC.planted_residual(case, fi, c.page, c.M, (qs, ts))
                got = VC.planted_residual(case, fi, c.page, a["transform"], (qs, ts))
                print("%s page %d: residual over the exact planted inliers %.3g px (restatement %.3g)" % (case.name, c.page, got, own))
                assert got <= 4 * own, (case.name, c.page, got, own)
    if stats:
        C.report("verify-stage reprojection " + case.name, **stats)


def test_search_engines_give_identical_records(capi):
    """Every case through the mfma2, mfma4 and valu search engines (the first two search the distinct rows and restore the twins,
    the third searches every row): byte-identical verdicts and candidate records."""
    for fa in CASES:
        case = VC.build(*fa)
        if len(case.frames) > 8:                    # (D3's 65 equal frames add nothing to a search comparison: its first two do)
            frames, kps, descs = _inputs(case)
            inputs = (frames[:2], kps[:2], descs[:2])
        else:
            inputs = _inputs(case)
        m, _ = _matcher(capi, case, small_cfg(capi, **case.cfg))
        got = []
        for e in ENGINES:
            m.set_knn_engine(e)
            v = m.match_features(*inputs)
            got.append((v, [m.last_candidates(i) for i in range(len(inputs[0]))]))
        m.close()
        for e, g in zip(ENGINES[1:], got[1:]):
            assert _same_records(got[0], g), "%s: %s differs from %s" % (case.name, e, ENGINES[0])


def test_tap_grows_the_rng_stream_itself(capi, monkeypatch):
    """A matcher that starts with 512 pre-drawn RNG outputs (SLIDEO_RNG_STREAM_LEN, read at creation): X1's candidate without a
    model and H1's five votes on one line sample until the iteration cap, far past them; the kernels raise the overflow flag and the
    tap draws more and runs its rows again (never through ORB): the records equal a default matcher's byte for byte."""
    for fa in ((VC.x1, ()), (VC.h1, (1,))):
        case = VC.build(*fa)
        cfg = small_cfg(capi, **case.cfg)
        m, _ = _matcher(capi, case, cfg)
        want = _run(m, case)
        m.close()
        monkeypatch.setenv("SLIDEO_RNG_STREAM_LEN", "512")
        m, _ = _matcher(capi, case, cfg)
        monkeypatch.delenv("SLIDEO_RNG_STREAM_LEN")
        got = _run(m, case)
        again = _run(m, case)                                   # (the stream has grown: no re-run now)
        m.close()
        assert _same_records(want, got) and _same_records(want, again), case.name


def test_tap_rejects_what_it_does_not_cover(capi):
    """SIFT mode, the LSH matcher and a matcher that is not finalized are refused; slideo_last_frame_candidates works after the tap
    (every other test of this module reads it)."""
    case = VC.build(VC.v3, ("tol",))
    frames, kps, descs = _inputs(case)
    m = capi.Matcher(small_cfg(capi))
    with pytest.raises(capi.SlideoError) as e:
        m.match_features(frames, kps, descs)
    assert e.value.code == 4                                   # SLIDEO_ERR_STATE: not finalized
    m.close()
    m = capi.Matcher(small_cfg(capi))
    m.use_sift(capi.sift_config(), 0.75)
    with pytest.raises(capi.SlideoError) as e:
        m.match_features(frames, kps, descs)
    assert e.value.code == 1                                   # SLIDEO_ERR_INVALID_ARG
    m.close()
    m = capi.Matcher(small_cfg(capi, matcher=1))
    p = case.pages[0]
    m.add_page_features(VC.PAGE_W, VC.PAGE_H, VC.keypoints(p.xy), p.desc, m.small_image(VC.page_image(p.img)))
    m.finalize()
    with pytest.raises(capi.SlideoError) as e:
        m.match_features(frames, kps, descs)
    assert e.value.code == 1
    m.close()
