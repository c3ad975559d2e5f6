"""Use and cost of the direct look-up scope SLIDEO_DIRECT_VALID (include/slideo_amd.h "Direct look-up scope") on the recording both
the frame mask's GATE scope and the direct page look-up were made for: the synthetic SCREEN RECORDING of tools/direct_rate.py (deck
pages reduced to 1080p plus noise, holds of geometric length, a share of the holds one of the generator's transformed frames) with the
speaker-sized inset of tools/gate_mask_rate.py (20 % of the frame, bottom right, a random binary texture, another one on EVERY
frame) on top.  500 pages, ORB-1000, 256 device-resident 1080p frames, gated submit / collect in units of 128, one process,
alternated repeats, min / median / max:

  choose  under the hole mask, the distribution of the masked s_i (numpy over the masked tap's SSDs, normalised over n_valid) of the
          full-screen frames, of the transformed frames and of the full-screen frames' nearest WRONG page: what a user needs to
          choose t; beside it the full-screen frames' WHOLE-image similarity (what SLIDEO_DIRECT_WHOLE would compare)
  use     (a) DETECT | GATE, t = 0: what a user of this recording can do today
          (b) DETECT | GATE, SLIDEO_DIRECT_VALID, t = --t
          (c) DETECT alone, SLIDEO_DIRECT_WHOLE, the same t: today's other option
          and the share of changed frames resolved directly in (b) and in (c), and whether every direct verdict names the page shown

    python tools/direct_mask_rate.py [--share 0.5] [--moved 0.25] [--frames 256] [--pages 500] [--noise 3] [--t 0.9] [--reps 5]
                                     [--kernels-only] [--step-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: the gated stream twice as (b) and twice without a
mask under SLIDEO_DIRECT_WHOLE at the same t, and nothing else, for a profiler's kernel trace of its own
(the weighted direct_centre_kernel instances beside the unweighted one on the same units).  --step-only: the gated stream as (a) alone, through no
call an older library lacks (SLIDEO_LIB_PATH: the parent commit's build, interleaved process by process as tools/ab_libs.sh does)."""
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
from direct_rate import recording, similarity, mmm  # noqa: E402
from frame_mask_rate import inset_rect  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
UNIT = 128
DET, BOTH = _capi.MASK_DETECT, _capi.MASK_DETECT | _capi.MASK_GATE


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
    y0, x0 = inset_rect(W, H)
    hole = np.full((H, W), 255, np.uint8)
    hole[y0:, x0:] = 0
    d = torch.from_numpy(seq).cuda()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261018)
    d[:, y0:, x0:] = torch.randint(0, 2, (N, H - y0, W - x0, 1), device="cuda", generator=gen, dtype=torch.uint8) * 255
    fbb = W * H * 3
    res = {"shape": "%d pages, %d 1080p frames, ORB-1000, holds geometric with mean %.1f, %.0f %% of the holds transformed, noise +-%d; "
                    "inset %dx%d at (%d, %d), another one per frame" % (a.pages, N, 1 / a.share, 100 * a.moved, a.noise, W - x0, H - y0, x0, y0),
           "lib": os.environ.get("SLIDEO_LIB_PATH", "product")}

    def gated():
        m.gate_reset(None)
        out = []
        stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fbb, c, W, H), lambda t: out.append(m.collect_changed(t)), N, UNIT)
        return np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out])

    def setup(mask_scope, mask, direct_scope, t):
        """One of the tool's configurations, from any other: through t = 0 and no mask, so that no set call refuses."""
        m.set_direct_similarity(0.0)
        m.set_frame_mask(None)
        m.set_frame_mask_scope(mask_scope)
        if direct_scope is not None:
            m.set_direct_scope(direct_scope)
        m.set_frame_mask(mask)
        if t:
            m.set_direct_similarity(t)

    def timed(runs, reps):
        for prep, fn in runs.values():
            prep()
            fn()                                                                # (warm: workspaces sized, operand and norms built)
        t = {k: [] for k in runs}
        for _ in range(reps):                                                   # (alternating, so that clock and thermal drift hit all alike)
            for k, (prep, fn) in runs.items():
                prep()
                t0 = time.perf_counter()
                fn()
                t[k].append(time.perf_counter() - t0)
        return {k: mmm(v) for k, v in t.items()}

    def report(name, r):
        print("%-30s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s (of the stream)"
              % (name, r["min"], r["median"], r["max"], N, N / (r["median"] * 1e-3)), flush=True)

    if a.step_only:
        m.set_frame_mask_scope(BOTH)
        m.set_frame_mask(hole)
        r = timed({"a_gate_t0": (lambda: None, gated)}, a.reps)["a_gate_t0"]
        report("a_gate_t0", r)
        res["a_gate_t0_ms"] = r
        m.close()
        print(json.dumps(res))
        return
    if a.kernels_only:
        for cfg in ((BOTH, hole, _capi.DIRECT_VALID, a.t), (DET, None, _capi.DIRECT_WHOLE, a.t)) * 2:
            setup(*cfg)
            gated()
        m.close()
        return

    # ---- choose: the masked similarities of this content, from the masked tap -------------------------------------------------
    setup(BOTH, hole, None, 0.0)
    valid, n_valid = m.frame_mask_small()
    first = starts                                                              # one frame per hold
    smalls = np.stack([m.small_image(d[i].cpu().numpy()) for i in first])
    ssd = m.page_small_ssd_valid(smalls).astype(np.float64)
    whole = m.page_small_ssd(smalls).astype(np.float64)
    npx = smalls.shape[1] * smalls.shape[2]
    best, arg = ssd.min(axis=1), ssd.argmin(axis=1)
    s_best = similarity(best, n_valid)
    tr = truth[first]
    fs, mv = tr >= 0, tr < 0
    wrong = ssd.copy()
    wrong[np.arange(len(first))[fs], tr[fs]] = np.inf
    s_wrong = similarity(wrong[fs].min(axis=1), n_valid)
    s_whole = similarity(whole.min(axis=1), npx)

    def dist(x):
        return {"min": float(np.min(x)), "p05": float(np.percentile(x, 5)), "median": float(np.median(x)), "p95": float(np.percentile(x, 95)),
                "max": float(np.max(x))} if len(x) else None
    res["choose"] = {"n_valid": n_valid, "n_pixels": npx, "holds_full_screen": int(fs.sum()), "holds_transformed": int(mv.sum()),
                     "s_full_screen": dist(s_best[fs]), "s_transformed": dist(s_best[mv]), "s_full_screen_nearest_wrong_page": dist(s_wrong),
                     "s_full_screen_whole_image": dist(s_whole[fs]), "full_screen_argmin_is_the_page": bool((arg[fs] == tr[fs]).all())}
    for k in ("s_full_screen", "s_transformed", "s_full_screen_nearest_wrong_page", "s_full_screen_whole_image"):
        print("choose: %-34s %s" % (k, res["choose"][k]), flush=True)

    # ---- use ------------------------------------------------------------------------------------------------------------------
    conf = {"a_gate_t0": (BOTH, hole, _capi.DIRECT_WHOLE, 0.0), "b_gate_valid_t": (BOTH, hole, _capi.DIRECT_VALID, a.t),
            "c_detect_whole_t": (DET, hole, _capi.DIRECT_WHOLE, a.t)}
    res["use"] = {"t": a.t}
    out = {}
    for k, cfg in conf.items():
        setup(*cfg)
        c, v = gated()
        direct = c & (v["page_idx"] >= 0) & (v["inliers"] == 0)
        out[k] = (c, v, direct)
        res["use"][k] = {"changed_share": float(c.mean()), "direct_share_of_changed": float(direct.sum() / max(int(c.sum()), 1)),
                         "direct_verdicts_name_the_shown_page": bool((v["page_idx"][direct] == truth[direct]).all()),
                         "transformed_frames_direct": int((direct & (truth < 0)).sum())}
        print("use: %-18s %s" % (k, res["use"][k]), flush=True)
    ca, va, _ = out["a_gate_t0"]
    cb, vb, db = out["b_gate_valid_t"]
    assert np.array_equal(ca, cb), "the flags depend neither on t nor on the direct scope"
    res["use"]["b_pipeline_verdicts_equal_a"] = bool(va[cb & ~db].tobytes() == vb[cb & ~db].tobytes())
    t = timed({k: ((lambda cfg=cfg: setup(*cfg)), gated) for k, cfg in conf.items()}, a.reps)
    res["use"]["ms"] = t
    for k, r in t.items():
        report("use: " + k, r)
    res["use"]["a_over_b"] = t["a_gate_t0"]["median"] / t["b_gate_valid_t"]["median"]
    res["use"]["c_over_b"] = t["c_detect_whole_t"]["median"] / t["b_gate_valid_t"]["median"]
    print("use: (a) / (b) %.2fx, (c) / (b) %.2fx" % (res["use"]["a_over_b"], res["use"]["c_over_b"]), flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
