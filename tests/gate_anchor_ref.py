"""The gate reference SLIDEO_GATE_ANCHOR (include/slideo_amd.h "Gate reference") restated in numpy, on gate_mask_ref's similarity,
masked SSD and threshold: a frame is compared with the ANCHOR — the last frame that was flagged — not with the frame before it.
Nothing here calls the library under test."""
import numpy as np

import gate_mask_ref as gref


def flags(smalls, valid, changed_similarity, anchor_small=None):
    """The anchor rule over small images under the validity map (None: whole images)
    -> (changed bool [n], similarity f32 [n], anchor int [n], last anchor small image or None).
    anchor[i]: the frame f_i was compared with, -1 = the carried anchor `anchor_small`; without one (the state "none") frame 0
    compares as 0.0 against nothing (-1), is changed and becomes the anchor."""
    if valid is None:
        valid = np.ones(smalls.shape[1:3], bool)
    n = int(valid.sum())
    ch = np.zeros(len(smalls), bool)
    sim = np.zeros(len(smalls), np.float32)
    ref = np.full(len(smalls), -1, np.int64)
    anchor, at = anchor_small, -1
    for i, s in enumerate(smalls):
        ref[i] = at
        sim[i] = np.float32(0.0) if anchor is None else gref.similarity(gref.masked_ssd(anchor, s, valid), n)
        ch[i] = sim[i] < np.float32(changed_similarity)
        if ch[i]:
            anchor, at = s, i
    return ch, sim, ref, anchor


def all_pairs_ssd(smalls, valid=None):
    """int64 [n, n]: the SSD of every pair of small images over the valid pixels (None: whole images), exact."""
    x = smalls.reshape(len(smalls), -1, 3)
    if valid is not None:
        x = x[:, np.asarray(valid).reshape(-1)]
    x = x.reshape(len(x), -1)
    # <x_i, x_j> in float64, K chunk by K chunk: every product is an integer <= 255^2 and every sum stays below 2^53 (255^2 * 2^16
    # per chunk), so the matrix product is exact; the chunks are added in int64
    dot = np.zeros((len(x), len(x)), np.int64)
    for k in range(0, x.shape[1], 1 << 16):
        c = x[:, k:k + (1 << 16)].astype(np.float64)
        dot += np.rint(c @ c.T).astype(np.int64)
    sq = np.diagonal(dot)
    return sq[:, None] + sq[None, :] - 2 * dot


def walk(table, carried, thr, none):
    """The rule in integers over a table of SSDs: table[a][j] for frames a < j of one unit, carried[j] against the carried anchor;
    flagged iff ssd >= thr; none: the state "none" (frame 0 flagged with SSD 0).
    -> (flags [n] uint8, ssd [n] int64 against each frame's anchor, the last flagged frame or -1)."""
    n = len(carried)
    fl = np.zeros(n, np.uint8)
    ssd = np.zeros(n, np.int64)
    a = -1
    for j in range(n):
        if none and j == 0:
            s, hit = 0, True
        else:
            s = int(carried[j]) if a < 0 else int(table[a][j])
            hit = s >= thr
        ssd[j] = s
        if hit:
            fl[j] = 1
            a = j
    return fl, ssd, a
