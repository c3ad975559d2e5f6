"""Walk cases for the gate memory (include/slideo_amd.h "Gate memory"), shared by tests/test_gate_memory_abi.py (the host check's case
file) and tests/test_gpu_gate_memory_kernels.py (slideo_gate_recall_walk): frames and memory entries as integer vectors of 8
components, as tests/test_gpu_gate_settle_kernels.py builds its own, so that the tables of dot products and norms are exact integers.
A case is a dict of everything the tap takes plus the SSD tables the restatement (tests/gate_memory_ref.py walk) takes."""
import functools

import numpy as np

import gate_memory_ref as mref

NS = [1, 2, 63, 64, 65, 130, 300]
MS = [1, 2, 3, 64]
STATES = ["none", "partial", "full"]
SETTLES = [None, 0, 4, 2 ** 30]                                  # None: no settle; else the cap under a settle
INT64_MAX = (1 << 63) - 1
THR_S = 8 * 2 * 2 + 1                                            # steps of at most 2 per component are still


def _ring(M, state, rng):
    """-> (count, head, anchor slot, ordinals [M], t0): the ring a state kernel leaves."""
    if state == "none":
        return 0, 0, 0, np.zeros(M, np.int64), 0
    if state == "partial":
        count = max(1, M // 2)
        head = count % M
        ords = np.zeros(M, np.int64)
        ords[:count] = 100 + 3 * np.arange(count)
        if count > 1:
            ords[0] = mref.REF_RESET                             # the oldest entry is a reset's image
        return count, head, int(rng.integers(0, count)), ords, 100 + 3 * count + 5
    head = M // 2 if M > 1 else 0                                # full; head is the oldest slot
    ords = 1000 + 2 * ((np.arange(M) - head) % M)
    return M, head, int(rng.integers(0, M)), ords.astype(np.int64), 1000 + 2 * M + 7


def tables(x, mem):
    """Frames x [n, 8] and memory slots mem [M, 8] -> dot, norm, mdot, mnorm, SSD table [n, n], SSD mtable [n, M]."""
    x, mem = x.astype(np.int64), mem.astype(np.int64)
    dot, norm = x @ x.T, (x * x).sum(axis=1)
    mdot, mnorm = x @ mem.T, (mem * mem).sum(axis=1)
    return dot, norm, mdot, mnorm, norm[:, None] + norm[None, :] - 2 * dot, norm[:, None] + mnorm[None, :] - 2 * mdot


def make(x, mem, M, ring, thr_c, thr_s, max_defer, d_in, prev, what):
    count, head, anchor, ords, t0 = ring
    dot, norm, mdot, mnorm, table, mtable = tables(x, mem)
    none = count == 0
    prev_ssd0 = int(((prev.astype(np.int64) - x[0]) ** 2).sum())
    c = dict(what=what, n=len(x), M=M, dot=dot, norm=norm, mdot=mdot, mnorm=mnorm, table=table, mtable=mtable, ordinals=ords, count=count, head=head,
             anchor=anchor, prev_ssd0=prev_ssd0, thr_c=int(thr_c), thr_s=int(thr_s), max_defer=int(max_defer), d_in=0 if none else int(d_in), none=none,
             t0=t0)
    c["want"] = mref.walk(table, mtable, ords, count, head, anchor, prev_ssd0, c["thr_c"], c["thr_s"], c["max_defer"], c["d_in"], none, t0, M)
    return c


def stream_case(n, M, state, settle, seed):
    """A "revisit" stream: holds of a few pictures (small steps: still, not away), hard cuts and returns to pictures shown before —
    among them the carried entries' —, and fades (large steps: away, not still).  More pictures than slots, so entries are evicted."""
    rng = np.random.default_rng(seed)
    ring = _ring(M, state, rng)
    count = ring[0]
    n_pic = min(M, 6) + 3
    pics = 1000 + 400 * rng.integers(-5, 6, (n_pic, 8))
    mem = 1000 + 400 * rng.integers(-5, 6, (M, 8)) + 7           # unoccupied slots: anything
    for c in range(count):
        mem[c] = pics[c % n_pic] + rng.integers(-1, 2, 8)        # carried entries show pictures of the stream
    x = np.zeros((n, 8), np.int64)
    cur = pics[int(rng.integers(0, n_pic))]
    j = 0
    while j < n:
        u = rng.random()
        if u < 0.55:                                             # a hold under noise
            for _ in range(int(rng.integers(1, 7))):
                if j < n:
                    x[j] = cur + rng.integers(-1, 2, 8)
                    j += 1
        elif u < 0.85:                                           # a hard cut, often back to an earlier picture
            cur = pics[int(rng.integers(0, n_pic))]
        else:                                                    # a fade to another picture
            nxt = pics[int(rng.integers(0, n_pic))]
            steps = int(rng.integers(3, 9))
            for k in range(1, steps):
                if j < n:
                    x[j] = cur + (nxt - cur) * k // steps
                    j += 1
            cur = nxt
    thr_c = 8 * 30 * 30                                          # noise of +-1 (+-2 against a noisy entry) is far inside, a step between pictures far outside
    max_defer = 0 if settle is None else settle
    d_in = min(max_defer, 3) if seed % 2 else 0
    prev = x[0] + rng.integers(-1, 2, 8) if seed % 3 else x[0] + 300
    return make(x, mem, M, ring, thr_c, THR_S if settle is not None else 0, max_defer, d_in, prev,
                "stream n=%d M=%d %s settle=%s" % (n, M, state, settle))


@functools.lru_cache(maxsize=None)
def all_stream_cases():
    out, seed = [], 0
    for n in NS:
        for M in MS:
            for state in STATES:
                for settle in SETTLES:
                    out.append(stream_case(n, M, state, settle, seed))
                    seed += 1
    return out


@functools.lru_cache(maxsize=None)
def forced_cases():
    """Tables that force one thing each; `what` names it."""
    out = []
    rng = np.random.default_rng(77)
    base = 1000 + 400 * rng.integers(-5, 6, (8, 8))
    far = base[7]
    # exact SSD ties between two entries: two carried slots hold the SAME vector under different ordinals, in both slot orders
    for M, ords in ((3, [40, 50, 60]), (3, [50, 40, 60]), (64, None)):
        mem = np.tile(far, (M, 1)) + 400 * (1 + np.arange(M))[:, None]
        mem[0], mem[1], mem[2] = base[0], base[0], base[1]
        o = np.arange(M, dtype=np.int64) * 2 + 10 if ords is None else np.array(ords, np.int64)
        if ords is None:
            mem[M - 1], o[M - 1], o[0], o[1] = base[0], 5000, 11, 9      # three equal entries: the greatest ordinal is in the last lane
        ring = (M, 0, 2, o, 7000)
        x = np.stack([base[1], base[0], base[0] + 1, base[1], base[0]])
        out.append(make(x, mem, M, ring, 8 * 30 * 30, 0, 0, 0, x[0], "tie between entries M=%d %s" % (M, ords)))
    # a tie with the threshold: the best entry at exactly T_c - 1 (recalled) and at exactly T_c (not recalled)
    for M in (2, 64):
        mem = np.tile(far, (M, 1)) + 400 * (1 + np.arange(M))[:, None]
        mem[0], mem[1] = base[0], base[1]
        ring = (2, 2 % M, 0, np.concatenate([[3, 4], np.zeros(M - 2, np.int64)]).astype(np.int64), 50)
        step = np.array([9, 0, 0, 0, 0, 0, 0, 0])
        x = np.stack([base[0], base[1] + step, base[1] + step, base[0]])
        for thr_c, name in ((82, "T_c - 1"), (81, "T_c")):
            out.append(make(x, mem, M, ring, thr_c, 0, 0, 0, x[0], "best entry at %s M=%d" % (name, M)))
    # more than M matches in one unit, then a return to an evicted and to a surviving in-unit entry; from "none" and from a full ring
    for M in (2, 3):
        for state in ("none", "full"):
            ring = _ring(M, state, rng)
            mem = np.tile(far, (M, 1)) + 400 * (1 + np.arange(M))[:, None]
            order = list(range(M + 2)) + [0, M + 1, 1, M]        # pictures 0 .. M + 1 matched, then 0 (evicted), M + 1 (survives), 1, M
            x = np.stack([base[k] + d for k in order for d in (0, 1)])
            out.append(make(x, mem, M, ring, 8 * 30 * 30, 0, 0, 0, x[0], "in-unit eviction M=%d %s" % (M, state)))
    # a recall of a carried entry, then frames compared against that carried anchor (unchanged under noise), across a 64-lane window
    for M in (3, 64):
        mem = np.tile(far, (M, 1)) + 400 * (1 + np.arange(M))[:, None]
        mem[0], mem[1] = base[0], base[1]
        ring = (2, 2 % M, 1, np.concatenate([[3, 4], np.zeros(M - 2, np.int64)]).astype(np.int64), 50)
        x = np.stack([base[1]] * 2 + [base[0] + (k % 3 - 1) for k in range(80)] + [base[1], base[2], base[0]])
        out.append(make(x, mem, M, ring, 8 * 30 * 30, 0, 0, 0, x[0], "carried recall then carried anchor M=%d" % M))
    # all frames away and deferred (nothing is within T_c = 0 of anything, nothing is still, the cap is never reached); no frame away
    for n in (65, 130):
        M = 3
        ring = _ring(M, "partial", rng)
        mem = 1000 + 400 * rng.integers(-5, 6, (M, 8))
        x = 1000 + np.cumsum(rng.integers(-40, 41, (n, 8)), axis=0)
        out.append(make(x, mem, M, ring, 0, 0, 2 ** 30, 2, x[0] + 300, "all deferred n=%d" % n))
        out.append(make(x, mem, M, ring, INT64_MAX, THR_S, 4, 2, x[0], "none away n=%d" % n))
    return out
