"""Cost and use of the frame mask (include/slideo_amd.h "Frame mask") at the headline content (500 pages, ORB-1000, 256
device-resident 1080p frames per step), in one process, alternated repeats:

  step time      (a) no mask   (b) a mask with a speaker-sized hole (20 % of the frame, bottom right)
  truth share    on frames that carry a speaker inset (random binary texture over that 20 %): frames assigned to the synthetic
                 truth without and with the mask over the inset

    python tools/frame_mask_rate.py [--reps 5] [--frames 256] [--pages 500] [--kernels-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: two masked steps and nothing else (a short run to
trace mask_filter_kernel under rocprofv3 --kernel-trace --stats; a launch covers half of --frames: a step is two units)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slideo_amd import _capi, synth  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080


def inset_rect(w, h, share=0.2):
    """The bottom-right rectangle of `share` of a w x h frame, aspect kept: (y0, x0)."""
    s = share ** 0.5
    return h - int(round(h * s)), w - int(round(w * s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    B = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    frames, truth, _ = synth.frames(pages, B, W, H, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    y0, x0 = inset_rect(W, H)
    mask = np.full((H, W), 255, np.uint8)
    mask[y0:, x0:] = 0
    d = torch.from_numpy(frames).cuda()
    res = {"shape": "%d pages, %d frames of %dx%d, ORB-1000; hole %dx%d at (%d, %d)" % (a.pages, B, W, H, W - x0, H - y0, x0, y0)}

    def step(ptr, masked):
        m.set_frame_mask(mask if masked else None)
        return m.match_frames_dev(ptr, B, W, H)

    if a.kernels_only:
        for _ in range(2):
            step(d.data_ptr(), True)
        m.close()
        return

    runs = {"a_plain": lambda: step(d.data_ptr(), False), "b_masked": lambda: step(d.data_ptr(), True)}
    for fn in runs.values():
        fn()                                                                    # (warm: workspaces sized, the pyramid's geometry built)
    t = {k: [] for k in runs}
    for _ in range(a.reps):                                                     # (alternating, so that clock and thermal drift hit both alike)
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    for k in runs:
        med = float(np.median(t[k]))
        res["%s_ms" % k] = [x * 1e3 for x in t[k]]
        res["%s_fps" % k] = B / med
        print("%-9s %s ms (median %.2f, spread %.2f) = %.0f frames/s" % (k, " ".join("%.2f" % (x * 1e3) for x in t[k]), med * 1e3,
                                                                          (max(t[k]) - min(t[k])) * 1e3, B / med), flush=True)
    ma, mb = (float(np.median(t[k])) for k in ("a_plain", "b_masked"))
    res["masked_minus_plain_ms"] = (mb - ma) * 1e3
    res["plain_spread_ms"] = (max(t["a_plain"]) - min(t["a_plain"])) * 1e3
    print("masked - plain %.2f ms per %d frames; spread of plain %.2f ms" % ((mb - ma) * 1e3, B, res["plain_spread_ms"]), flush=True)

    # the speaker inset: random binary texture over the hole, another one per frame
    rng = np.random.default_rng(20261017)
    busy = frames.copy()
    for f in busy:
        f[y0:, x0:] = (rng.integers(0, 2, (H - y0, W - x0), dtype=np.uint8) * 255)[:, :, None]
    db = torch.from_numpy(busy).cuda()
    for name, masked in (("plain", False), ("masked", True)):
        v = step(db.data_ptr(), masked)
        res["inset_truth_share_%s" % name] = float((v["page_idx"] == truth).mean())
        res["inset_mean_keypoints_%s" % name] = float(v["n_keypoints"].mean())
        print("inset frames, %-6s: assigned to the truth %.4f, keypoints per frame %.0f"
              % (name, res["inset_truth_share_%s" % name], res["inset_mean_keypoints_%s" % name]), flush=True)
    v = step(d.data_ptr(), False)
    res["clean_truth_share"] = float((v["page_idx"] == truth).mean())
    print("the same frames without an inset, no mask: assigned to the truth %.4f" % res["clean_truth_share"], flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
