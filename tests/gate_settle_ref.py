"""The gate settle (include/slideo_amd.h "Gate settle") restated in numpy, on gate_mask_ref's similarity, masked SSD and threshold:
under the ANCHOR reference a frame that is away from the anchor is matched only once it is still — within settle_similarity of the
frame before it — or after max_defer deferred frames.  Nothing here calls the library under test."""
import numpy as np

import gate_mask_ref as gref

UNCHANGED, DEFERRED, MATCHED_STILL, MATCHED_CAP = 0, 1, 2, 3      # what happened to a frame (`kind`)


def decide(away, still, d, max_defer):
    """One frame of the rule -> (kind, the count behind it)."""
    if not away:
        return UNCHANGED, 0
    if still:
        return MATCHED_STILL, 0
    if d >= max_defer:
        return MATCHED_CAP, 0
    return DEFERRED, min(d + 1, max_defer)


def flags(smalls, valid, changed_similarity, settle_similarity, max_defer, state=None):
    """The settle rule over small images under the validity map (None: whole images), from `state` = (anchor small image, previous
    small image, d) or None (the state "none")
    -> (changed bool [n], similarity f32 [n], kind int [n], d int [n] (the count in front of each frame), state behind the stream)."""
    if valid is None:
        valid = np.ones(smalls.shape[1:3], bool)
    n = int(valid.sum())
    t_c, t_s = gref.threshold(changed_similarity, n), gref.threshold(settle_similarity, n)
    ch = np.zeros(len(smalls), bool)
    sim = np.zeros(len(smalls), np.float32)
    kind = np.zeros(len(smalls), np.int64)
    ds = np.zeros(len(smalls), np.int64)
    anchor, prev, d = state if state is not None else (None, None, 0)
    for i, s in enumerate(smalls):
        ds[i] = d
        if anchor is None:
            sim[i], kind[i], d = np.float32(0.0), MATCHED_STILL, 0
        else:
            ssd_a = gref.masked_ssd(anchor, s, valid)
            sim[i] = gref.similarity(ssd_a, n)
            kind[i], d = decide(ssd_a >= t_c, gref.masked_ssd(prev, s, valid) < t_s, d, max_defer)
        ch[i] = kind[i] >= MATCHED_STILL
        if ch[i]:
            anchor = s
        prev = s
    return ch, sim, kind, ds, (anchor, prev, d)


def walk(table, carried, thr_c, thr_s, max_defer, d_in, none):
    """The rule in integers over a table of SSDs: table[a][j] for frames a < j of one unit, carried[j] (j < n) against the carried
    anchor, carried[n] frame 0 against the carried previous frame; none: the state "none" (frame 0 matched with SSD 0).
    -> (flags [n] uint8, ssd [n] int64 against each frame's anchor, kind [n], the last matched frame or -1, the count behind)."""
    n = len(carried) - 1
    fl = np.zeros(n, np.uint8)
    ssd = np.zeros(n, np.int64)
    kind = np.zeros(n, np.int64)
    a, d = -1, (0 if none else int(d_in))
    for j in range(n):
        if none and j == 0:
            s, kind[j], d = 0, MATCHED_STILL, 0
        else:
            s = int(carried[j]) if a < 0 else int(table[a][j])
            p = int(carried[n]) if j == 0 else int(table[j - 1][j])
            kind[j], d = decide(s >= thr_c, p < thr_s, d, max_defer)
        ssd[j] = s
        if kind[j] >= MATCHED_STILL:
            fl[j] = 1
            a = j
    return fl, ssd, kind, a, d
