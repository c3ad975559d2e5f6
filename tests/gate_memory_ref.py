"""The gate memory (include/slideo_amd.h "Gate memory") restated in numpy, on gate_mask_ref's similarity, masked SSD and threshold:
under the ANCHOR reference, with or without a gate settle, the last M matched frames are remembered and a frame that is away from the
anchor but within changed_similarity of one of them is recalled — it stands behind that frame's verdict — instead of matched.
Nothing here calls the library under test."""
import numpy as np

import gate_mask_ref as gref

UNCHANGED, RECALLED, DEFERRED, MATCHED = 0, 1, 2, 3               # what happened to a frame (`kind`)
REF_RESET, REF_DEFERRED = -1, -2                                 # SLIDEO_GATE_REF_RESET, SLIDEO_GATE_REF_DEFERRED
SLOTS = 64                                                       # SLIDEO_GATE_MEMORY_MAX


def reset_state(small):
    """The state slideo_matcher_gate_reset(S) leaves: E = [(S, REF_RESET)], S anchor and previous frame, d = 0, next ordinal 0."""
    return [(small, REF_RESET)], 0, small, 0, 0


def best_entry(ssds, ordinals):
    """The entry with the smallest SSD, ties to the greatest ordinal -> its index."""
    return min(range(len(ssds)), key=lambda e: (int(ssds[e]), -int(ordinals[e])))


def flags(smalls, valid, changed_similarity, settle_similarity, max_defer, M, state=None):
    """The rule over small images under the validity map (None: whole images).  settle_similarity 0 / None: no settle (an away frame
    that is not recalled is matched at once).  state: None (the state "none") or (entries [(small image, ordinal)] oldest first, the
    anchor's index, the previous small image, d, the next ordinal)
    -> (changed bool [n], similarity f32 [n], kind int [n], refs int64 [n], state behind the stream)."""
    assert 1 <= M <= SLOTS
    if valid is None:
        valid = np.ones(smalls.shape[1:3], bool)
    n = int(valid.sum())
    settle = bool(settle_similarity)
    t_c = gref.threshold(changed_similarity, n)
    t_s = gref.threshold(settle_similarity, n) if settle else 0
    ch = np.zeros(len(smalls), bool)
    sim = np.zeros(len(smalls), np.float32)
    kind = np.zeros(len(smalls), np.int64)
    refs = np.zeros(len(smalls), np.int64)
    if state is None:
        E, a, prev, d, t = [], -1, None, 0, 0
    else:
        E, a, prev, d, t = list(state[0]), state[1], state[2], state[3], state[4]
    for i, s in enumerate(smalls):
        if not E:
            sim[i], kind[i] = np.float32(0.0), MATCHED
        else:
            ssd_a = gref.masked_ssd(E[a][0], s, valid)
            sim[i] = gref.similarity(ssd_a, n)
            if ssd_a < t_c:
                kind[i], d, refs[i] = UNCHANGED, 0, E[a][1]
            else:
                ssd_e = [gref.masked_ssd(e[0], s, valid) for e in E]
                r = best_entry(ssd_e, [e[1] for e in E])
                if ssd_e[r] < t_c:
                    kind[i], a, d, refs[i] = RECALLED, r, 0, E[r][1]
                elif not settle or gref.masked_ssd(prev, s, valid) < t_s or d >= max_defer:
                    kind[i] = MATCHED
                else:
                    kind[i], d, refs[i] = DEFERRED, min(d + 1, max_defer), REF_DEFERRED
        if kind[i] == MATCHED:
            ch[i] = True
            if len(E) == M:
                E.pop(0)                                         # FIFO: a recall does not refresh an entry
            E.append((s, t))
            a, d, refs[i] = len(E) - 1, 0, t
        prev = s
        t += 1
    return ch, sim, kind, refs, (E, a, prev, d, t)


def walk(table, mtable, ordinals, count, head, anchor_slot, prev_ssd0, thr_c, thr_s, max_defer, d_in, none, t0, M):
    """The same rule in integers over a unit's tables of SSDs, as a ring of M slots: table[a][j] for frames a < j of the unit,
    mtable[j][c] frame j against the carried slot c (c < count; head: the slot the next match overwrites), prev_ssd0 frame 0 against
    the carried previous frame; max_defer 0: no settle (or a cap of 0); none: the state "none" (frame 0 matched with SSD 0).
    -> (flags uint8 [n], ssd int64 [n] against the anchor in force before each frame, refs int64 [n], kind [n], occupants int32 [64]
    (the frame of the unit in each slot behind the unit, -1: what it carried or nothing), head, count, anchor slot, d)."""
    n = len(table)
    fl = np.zeros(n, np.uint8)
    ssd = np.zeros(n, np.int64)
    refs = np.zeros(n, np.int64)
    kind = np.zeros(n, np.int64)
    occ = np.full(SLOTS, -1, np.int32)
    if none:
        ords, count, head, a, d = [0] * M, 0, 0, 0, 0
    else:
        ords, a, d = [int(o) for o in ordinals], int(anchor_slot), min(int(d_in), max_defer)

    def against(slot, j):
        return int(mtable[j][slot]) if occ[slot] < 0 else int(table[occ[slot]][j])

    for j in range(n):
        matched = False
        if count == 0:
            s, matched = 0, True
        else:
            s = against(a, j)
            if s < thr_c:
                kind[j], d, refs[j] = UNCHANGED, 0, ords[a]
            else:
                e = [against(c, j) for c in range(count)]
                r = best_entry(e, ords[:count])
                p = int(prev_ssd0) if j == 0 else int(table[j - 1][j])
                if e[r] < thr_c:
                    kind[j], a, d, refs[j] = RECALLED, r, 0, ords[r]
                elif max_defer == 0 or p < thr_s or d >= max_defer:
                    matched = True
                else:
                    kind[j], d, refs[j] = DEFERRED, min(d + 1, max_defer), REF_DEFERRED
        ssd[j] = s
        if matched:
            kind[j], fl[j] = MATCHED, 1
            occ[head], ords[head] = j, t0 + j
            a, head, count, d, refs[j] = head, (head + 1) % M, min(count + 1, M), 0, t0 + j
    return fl, ssd, refs, kind, occ, head, count, a, d

