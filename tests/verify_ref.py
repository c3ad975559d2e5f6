"""The verify stage as a plain numpy statement: search, vote, candidates, rating, verdict (mo/lib.rs:268-389 as cited in
csrc/verify.hip.h).  Written from the rules, from neither implementation; the point-level estimator is a parameter (the tests pass
the restatement's estimate_affine_partial / find_homography, themselves pinned to OpenCV by test_opencv_pin and
test_oracle_homography) and the similarities the verdict rule reads are supplied by the caller.

    stage(cfg, train, train_page, page_xy, frame_xy, frame_desc, estimator) -> Stage
    verdict(cfg, stage, sims)                                                -> (page_idx, similarity, inliers, n_keypoints)
"""
from collections import namedtuple

import numpy as np

Candidate = namedtuple("Candidate", "page n_votes votes found M mask inliers")
# cands: candidate order; rated: candidate slots in rating order after the max_rated cut; surv: the slots of `rated` that survive
Stage = namedtuple("Stage", "n_keypoints cands rated surv")


def unpack(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1)


def hamming(q, t):
    """All distances [nq, nt] between 32-byte rows."""
    qb, tb = unpack(q).astype(np.float32), unpack(t).astype(np.float32)       # (sums of at most 256 ones: exact in f32)
    d = qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)
    return np.rint(d).astype(np.int64)


def knn(q, t, k):
    """Brute force: per query the first k of (distance ascending, train row ascending); -1 where there are fewer rows."""
    d = hamming(q, t)
    nq, nt = d.shape
    order = np.argsort(d, axis=1, kind="stable")[:, :k]                       # (stable: equal distances keep ascending rows)
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), -1, np.int64)
    m = min(k, nt)
    idx[:, :m] = order[:, :m]
    dist[:, :m] = np.take_along_axis(d, order[:, :m], axis=1)
    return idx, dist


def vote(cfg, idx, dist):
    """-> the votes as (query, train row) in the order query ascending then list rank ascending."""
    out = []
    k = idx.shape[1]
    for q in range(idx.shape[0]):
        if idx[q, 0] < 0:
            continue
        if cfg.ratio_test > 0:
            if k >= 2 and idx[q, 1] >= 0 and np.float32(dist[q, 0]) < np.float32(cfg.ratio_test) * np.float32(dist[q, 1]):
                out.append((q, int(idx[q, 0])))
            continue
        lim = np.float32(dist[q, 0]) * np.float32(cfg.vote_tolerance)
        for r in range(k):
            if idx[q, r] < 0 or not np.float32(dist[q, r]) < lim:
                break
            out.append((q, int(idx[q, r])))
    return out


def stage(cfg, train, train_page, page_xy, frame_xy, frame_desc, estimator):
    """train [M, 32], train_page [M], page_xy [M, 2] f32: the deck's rows in page order; frame_xy [K, 2] f32, frame_desc [K, 32]:
    one frame's features; estimator(from_xy, to_xy) -> (found, M 3x3, mask): from = slide points, to = frame points."""
    K = len(frame_desc)
    if K == 0:
        return Stage(0, [], [], [])
    idx, dist = knn(frame_desc, train, cfg.knn_k)
    per_page = {}
    for q, t in vote(cfg, idx, dist):
        per_page.setdefault(int(train_page[t]), []).append((q, t))
    pages = sorted(per_page, key=lambda p: (-len(per_page[p]), p))[:cfg.max_candidate_pages]
    cands = []
    for p in pages:
        v = per_page[p]
        frm = np.array([page_xy[t] for _, t in v], np.float32).reshape(-1, 2)
        to = np.array([frame_xy[q] for q, _ in v], np.float32).reshape(-1, 2)
        found, M, mask = estimator(frm, to)
        cands.append(Candidate(p, len(v), v, bool(found), np.asarray(M, np.float64).reshape(3, 3), np.asarray(mask, np.uint8),
                               int(np.asarray(mask).sum())))
    rated = sorted(range(len(cands)), key=lambda i: -cands[i].inliers)[:cfg.max_rated]       # (sorted is stable)
    surv = []
    if rated:
        best = float(cands[rated[0]].inliers)
        for i in rated:
            inl = float(cands[i].inliers)
            if inl > cfg.min_rating and best > 0 and inl / best > cfg.min_rating_ratio:
                surv.append(i)
    return Stage(K, cands, rated, surv)


def verdict(cfg, st, sims):
    """sims: candidate slot -> similarity (f32) of every survivor.  -> (page_idx, similarity, inliers, n_keypoints)."""
    pick = None
    if cfg.verdict_rule == 1:
        for i in st.surv:
            if np.float32(sims[i]) > np.float32(cfg.min_similarity):
                pick = i
                break
    else:
        for i in st.surv:                                      # the first maximal similarity in rating order
            if pick is None or np.float32(sims[i]) > np.float32(sims[pick]):
                pick = i
        if pick is not None and not np.float32(sims[pick]) > np.float32(cfg.min_similarity):
            pick = None
    if pick is None:
        return (-1, np.float32(0), 0, st.n_keypoints)
    return (st.cands[pick].page, np.float32(sims[pick]), st.cands[pick].inliers, st.n_keypoints)
