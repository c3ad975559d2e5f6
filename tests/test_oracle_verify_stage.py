"""The restatement's verify stage against its definition on constructed features (tests/verify_cases.py): PageDB.
match_features_trace — match_frame from the frame's features on — must equal tests/verify_ref.py on every case: candidates, votes,
inliers, survivors and verdicts exactly, transforms bit for bit (the estimator is the same function).  Also the builder's own
guards, and the planted-model recovery of the cases that plant one."""
import numpy as np
import pytest

import verify_cases as VC
import verify_ref as R
from conftest import small_cfg

CASES = VC.all_cases()


def _db(oracle, case, cfg):
    db = oracle.PageDB(cfg)
    smalls = {}
    for p in case.pages:
        if p.img not in smalls:
            smalls[p.img] = oracle.small_image(VC.page_image(p.img), cfg.small_area)
        db.add_page_features(VC.PAGE_W, VC.PAGE_H, VC.keypoints(p.xy), p.desc, smalls[p.img])
    assert db.finalize() == 0
    return db


@pytest.mark.parametrize("fa", CASES, ids=VC.case_id)
def test_restatement_equals_definition(oracle, fa):
    """Measured here (max residual of the estimator's model over the exact planted inliers, px): R2 refine 0: 4.6e-5 .. 9.4e-5, R2
    refine 10: 3.1e-5 .. 3.4e-5, H1 (every hdlt): 3.1e-5 .. 3.4e-5 — the f32 rounding of the planted points; R3: 0.50 at threshold 3,
    0.25 at 1.5 (its refit runs over the band points too, which pull it).  Printed per candidate with -s."""
    case = VC.build(*fa)
    cfg = small_cfg(oracle, **case.cfg)
    VC.check_guards(case, cfg.ransac_threshold)
    db = _db(oracle, case, cfg)
    ref = VC.reference(case, oracle, cfg)
    ofs = np.concatenate([[0], np.cumsum([len(p.xy) for p in case.pages])])
    for fi, f in enumerate(case.frames):
        ov, oc = db.match_features_trace(case.frame_pixels(fi), VC.keypoints(f.xy), f.desc)
        st = ref[fi]
        assert len(st.cands) <= 64
        assert list(oc["page_idx"]) == [c.page for c in st.cands]
        assert list(oc["n_votes"]) == [c.n_votes for c in st.cands]
        assert list(oc["inliers"]) == [c.inliers for c in st.cands]
        assert list(oc["survived"]) == [int(i in st.surv) for i in range(len(st.cands))]
        for a, c in zip(oc, st.cands):
            assert np.array_equal(a["transform"].reshape(3, 3), c.M, equal_nan=True), (case.name, c.page)
        sims = {i: oc["similarity"][i] for i in st.surv}
        page, sim, inl, nk = R.verdict(cfg, st, sims)
        assert (ov["page_idx"], ov["inliers"], ov["n_keypoints"]) == (page, inl, nk)
        assert ov["similarity"] == sim
        VC.check_expectations(case, fi, list(oc["page_idx"]), list(oc["n_votes"]), list(oc["inliers"]), list(oc["survived"]),
                              int(ov["page_idx"]))
        if "planted" in case.expect:
            for c in st.cands:
                if c.n_votes < 200:
                    continue
                # the vote order is the query order: the planted flags were recorded in it
                assert [q for q, _ in c.votes] == sorted(q for q, _ in c.votes)
                assert list(c.mask.astype(bool)) == f.planted[c.page], (case.name, c.page)
                qs = [q for q, _ in c.votes]; ts = [t - ofs[c.page] for _, t in c.votes]
                worst = VC.planted_residual(case, fi, c.page, c.M, (qs, ts))
                print("%s page %d: %d votes, %d inliers, max residual over the exact planted inliers %.3g px" %
                      (case.name, c.page, c.n_votes, c.inliers, worst))


def test_builder_guards_bite():
    """The guards are checks, not decoration: a near pair and a residual at the threshold are both refused."""
    c = VC.Case("guard", 1)
    pg = c.page(0)
    f = c.frame(0)
    c.link(f, pg, c.points(pg, 4))
    VC.check_guards(c, 3.0)
    c.pages[pg].desc[0] = c.frames[f].desc[1]                  # an unintended pair at distance 0
    with pytest.raises(AssertionError):
        VC.check_guards(c, 3.0)
    c = VC.Case("guard", 1)
    pg = c.page(0)
    f = c.frame(0)
    c.link(f, pg, c.points(pg, 4), disp=(3.02, 0.0))           # 0.02 px from the threshold
    with pytest.raises(AssertionError):
        VC.check_guards(c, 3.0)


def test_tolerance_rule_in_f32():
    """The vote rule's edges, d < best * tol in f32 and strict: 1.05f * 20 admits 20 not 21; * 40 admits 41 not 42; best 0 admits nothing."""
    tol = np.float32(1.05)
    for best, yes, no in ((20, 20, 21), (40, 41, 42), (19, 19, 20)):
        lim = np.float32(best) * tol
        assert np.float32(yes) < lim and not np.float32(no) < lim
    assert not np.float32(0) < np.float32(0) * tol
