"""Use and cost of the direct page look-up (include/slideo_amd.h "Direct page look-up") on a synthetic SCREEN RECORDING: 500 pages,
ORB-1000, 256 device-resident 1080p frames, holds of geometric length (mean 1 / --share).  A hold shows either a deck page reduced
to 1080p (the frame IS the slide) plus noise of +- --noise grey levels, another draw per hold, or — a share --moved of the holds —
one of the generator's transformed frames, so that the pipeline still has work.  One process, alternated repeats, min / median / max:

  choose  for this content, the distribution of s_i (numpy over the tap's SSDs) of the full-screen frames and of the transformed
          frames, and the full-screen frames' gap to the nearest WRONG page: what a user needs to choose t
  use     the gated stream (submit / collect, units of 128) with t = 0 against t = --t on the same flags, the share of changed
          frames that are direct, and whether every direct verdict names the page its hold shows
  model   the time that the page operand's bytes / HBM rate and the look-up's MACs / int8 rate give, beside the kernels (run with
          --kernels-only under a profiler's kernel trace for the kernels alone)

    python tools/direct_rate.py [--share 0.5] [--moved 0.25] [--frames 256] [--pages 500] [--noise 3] [--t 0.9] [--reps 5]
                                [--kernels-only] [--step-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: the gated stream twice with t = 0 and twice with t > 0
and nothing else.  --step-only: the gated stream with t = 0 alone, through no call an older library lacks (SLIDEO_LIB_PATH: the
parent commit's build, interleaved process by process as tools/ab_libs.sh does)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from slideo_amd import _capi, synth  # noqa: E402
from changed_gate_rate import stream  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
UNIT = 128
HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak
INT8_MACS_PER_S = 2.3e15            # dense int8 matrix peak, in multiply-accumulates


def mmm(ts):
    ms = sorted(x * 1e3 for x in ts)
    return {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}


def similarity(ssd, n):
    """The host expression (csrc/runtime.hpp changed_similarity) in numpy."""
    e = np.sqrt(np.asarray(ssd, np.float64))
    max_error = np.sqrt(np.float32(np.float32(255.0) * np.float32(255.0) * np.float32(3.0)) * np.float32(n))
    return np.float32(1.0) - e.astype(np.float32) / max_error


def recording(m, pages, n, share, moved, noise, seed=20261017):
    """-> (frames [n, H, W, 3], truth [n]: the page a full-screen hold shows, -1 for a transformed frame)."""
    rng = np.random.default_rng(seed)
    starts, i = [], 0
    while i < n:
        starts.append(i)
        i += int(rng.geometric(share))
    is_moved = rng.random(len(starts)) < moved
    base, _, _ = synth.frames(pages, int(is_moved.sum()) + 1, W, H, threads=NCPU)
    seq, truth, k = np.empty((n, H, W, 3), np.uint8), np.full(n, -1, np.int32), 0
    for j, s in enumerate(starts):
        e = starts[j + 1] if j + 1 < len(starts) else n
        if is_moved[j]:
            seq[s:e] = base[k]
            k += 1
        else:
            p = int(rng.integers(0, len(pages)))
            img = m.reduce(pages[p], W, H).astype(np.int16) + rng.integers(-noise, noise + 1, (H, W, 3))
            seq[s:e] = np.clip(img, 0, 255).astype(np.uint8)
            truth[s:e] = p
    return seq, truth, np.array(starts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--moved", type=float, default=0.25)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--noise", type=int, default=3)
    ap.add_argument("--t", type=float, default=0.9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    N = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    seq, truth, starts = recording(m, pages, N, a.share, a.moved, a.noise)
    d = torch.from_numpy(seq).cuda()
    fbb = W * H * 3
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, holds geometric with mean %.1f, %.0f %% of the holds transformed, noise +-%d"
                    % (a.pages, N, 1 / a.share, 100 * a.moved, a.noise), "lib": os.environ.get("SLIDEO_LIB_PATH", "product")}

    def gated():
        m.gate_reset(None)
        out = []
        stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fbb, c, W, H), lambda t: out.append(m.collect_changed(t)), N, UNIT)
        return np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out])

    def timed(runs, reps):
        for prep, fn in runs.values():
            prep()
            fn()                                                                # (warm: workspaces sized, the operand built)
        t = {k: [] for k in runs}
        for _ in range(reps):                                                   # (alternating, so that clock and thermal drift hit all alike)
            for k, (prep, fn) in runs.items():
                prep()
                t0 = time.perf_counter()
                fn()
                t[k].append(time.perf_counter() - t0)
        return {k: mmm(v) for k, v in t.items()}

    def report(name, r):
        print("%-22s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
              % (name, r["min"], r["median"], r["max"], N, N / (r["median"] * 1e-3)), flush=True)

    if a.step_only:
        r = timed({"gated_t0": (lambda: None, gated)}, a.reps)["gated_t0"]
        report("gated_t0", r)
        res["gated_t0_ms"] = r
        m.close()
        print(json.dumps(res))
        return
    if a.kernels_only:
        for t in (0.0, a.t) * 2:
            m.set_direct_similarity(t)
            gated()
        m.close()
        return

    # ---- choose: the similarities of this content, from the tap ---------------------------------------------------------------
    first = starts                                                              # one frame per hold
    smalls = np.stack([m.small_image(seq[i]) for i in first])
    ssd = m.page_small_ssd(smalls).astype(np.float64)
    npx = smalls.shape[1] * smalls.shape[2]
    best, arg = ssd.min(axis=1), ssd.argmin(axis=1)
    s_best = similarity(best, npx)
    tr = truth[first]
    fs, mv = tr >= 0, tr < 0
    wrong = ssd.copy()
    wrong[np.arange(len(first))[fs], tr[fs]] = np.inf
    s_wrong = similarity(wrong[fs].min(axis=1), npx)

    def dist(x):
        return {"min": float(np.min(x)), "p05": float(np.percentile(x, 5)), "median": float(np.median(x)), "p95": float(np.percentile(x, 95)),
                "max": float(np.max(x))} if len(x) else None
    res["choose"] = {"holds_full_screen": int(fs.sum()), "holds_transformed": int(mv.sum()), "s_full_screen": dist(s_best[fs]),
                     "s_transformed": dist(s_best[mv]), "s_full_screen_nearest_wrong_page": dist(s_wrong),
                     "full_screen_argmin_is_the_page": bool((arg[fs] == tr[fs]).all())}
    for k in ("s_full_screen", "s_transformed", "s_full_screen_nearest_wrong_page"):
        print("choose: %-34s %s" % (k, res["choose"][k]), flush=True)

    # ---- use: t = 0 against t > 0 on the same flags ---------------------------------------------------------------------------
    m.set_direct_similarity(0.0)
    c0, v0 = gated()
    m.set_direct_similarity(a.t)
    c1, v1 = gated()
    assert np.array_equal(c0, c1), "the flags do not depend on t"
    direct = c1 & (v1["page_idx"] >= 0) & (v1["inliers"] == 0)
    res["use"] = {"t": a.t, "changed_share": float(c0.mean()), "direct_share_of_changed": float(direct.sum() / max(int(c0.sum()), 1)),
                  "direct_verdicts_name_the_shown_page": bool((v1["page_idx"][direct] == truth[direct]).all()),
                  "transformed_frames_direct": int((direct & (truth < 0)).sum()),
                  "pipeline_verdicts_equal_t0": bool(v0[c1 & ~direct].tobytes() == v1[c1 & ~direct].tobytes())}
    print("use: %s" % res["use"], flush=True)
    t = timed({"gated_t0": (lambda: m.set_direct_similarity(0.0), gated), "gated_t": (lambda: m.set_direct_similarity(a.t), gated)}, a.reps)
    res["use"]["ms"] = t
    for k, r in t.items():
        report("use: " + k, r)
    res["use"]["t0_over_t"] = t["gated_t0"]["median"] / t["gated_t"]["median"]
    print("use: t = 0 / t = %.2f: %.2fx" % (a.t, res["use"]["t0_over_t"]), flush=True)

    # ---- model ----------------------------------------------------------------------------------------------------------------
    L = 3 * npx
    macs = float(N) * a.pages * L
    res["model"] = {"page_operand_bytes": a.pages * L, "macs": macs, "hbm_ms": a.pages * L / HBM_BYTES_PER_S * 1e3,
                    "int8_ms": macs / INT8_MACS_PER_S * 1e3}
    print("model: operand %.0f MB / HBM rate = %.3f ms; %.2e MACs / int8 rate = %.3f ms per %d frames"
          % (a.pages * L / 1e6, res["model"]["hbm_ms"], macs, res["model"]["int8_ms"], N), flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
