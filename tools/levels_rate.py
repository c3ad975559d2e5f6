"""Cost and use of the frame levels (include/slideo_amd.h "Frame levels").  One process per mode:

  --kernels   128 device-resident 1080p frames through the observe call with a content session open, three times each: (a) BGR frames
              under a table — levels_kernel OUT OF PLACE, out of the caller's memory into the staging; (b) planar RGB frames under
              the same table — pixels_to_bgr_kernel<PLANAR>, the yardstick (6 B per pixel, the same thread shape), then levels_kernel
              IN PLACE on what it wrote.  --content noise | slide chooses the pixels (the table's LDS look-ups broadcast on a slide).
              The observe driver cuts a call into blocks of at most 256 MiB of staging: a kernel's time per 128 frames is the sum of
              its launches of one call.  Run it under a profiler's kernel trace with statistics, in a run of its own.
  --hist      the same frames, no table, a levels and a content session open: levels_hist_kernel beside content_kernel, the
              yardstick (3 B per pixel in, the same frame walk), three calls of 128 frames.  --content slide (one synthetic frame
              repeated: every dword repeats frame after frame) | noise | constant (every sample in one bin).
  --use       the use case at the headline deck size: --pages synthetic pages of 2001 x 1125, ORB-1000, 32 frames at 1080p, darkened
              as clip(f32(frame) * gain * cast + offset): right pages and refusals without levels and with the table learnt from the
              darkened frames' own histogram at 1 % per end.

    python tools/levels_rate.py --kernels [--content noise] | --hist [--content slide] | --use [--pages 24]

Prints one line per measurement and, for --use, a JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from slideo_amd import _capi, matching, synth  # noqa: E402
from yuv_desc_rate import deck, W, H, NCPU  # noqa: E402

N = 128


def content(kind):
    """[N, H, W, 3] uint8 on the device, and the same as host array of one frame."""
    if kind == "noise":
        return torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda")
    if kind == "constant":
        return torch.full((N, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    pages = synth.pages(2, 2001, 1125, threads=NCPU)
    frames, _, _ = synth.frames(pages, 2, W, H, threads=NCPU)
    return torch.from_numpy(frames[1]).cuda()[None].expand(N, H, W, 3).contiguous()


def _timed(tag, fn):
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        print("%s: observe call of %d frames %.1f ms" % (tag, N, (time.perf_counter() - t0) * 1e3), flush=True)


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    d = content(a.content)
    planar = d.permute(0, 3, 1, 2).flip(1).contiguous()              # [N, 3, H, W], R G B planes
    torch.cuda.synchronize()
    lut = _capi.frame_levels_lut([34] * 3, [106] * 3)
    m.set_frame_levels(lut)
    m.content_begin(24)
    _timed("kernels %s: bgr, levels out of place" % a.content, lambda: m.observe_frames_dev(d.data_ptr(), N, W, H))
    m.set_pixel_format("planar_rgb")
    _timed("kernels %s: planar rgb, convert + levels in place" % a.content, lambda: m.observe_frames_dev(planar.data_ptr(), N, W, H))
    m.content_end()
    m.close()


def hist(a):
    m = _capi.Matcher(_capi.default_config())
    d = content(a.content)
    torch.cuda.synchronize()
    m.content_begin(24)
    m.levels_begin()
    _timed("hist %s" % a.content, lambda: m.observe_frames_dev(d.data_ptr(), N, W, H))
    h = m.levels_histogram()
    print("hist %s: %d samples per channel, %d bins in use" % (a.content, int(h[0].sum()), int((h > 0).sum())), flush=True)
    m.levels_end()
    m.content_end()
    m.close()


DARKENINGS = [("as generated", 1.0, 0.0, (1.0, 1.0, 1.0)), ("gain 0.7", 0.7, 0.0, (1.0, 1.0, 1.0)), ("gain 0.5", 0.5, 0.0, (1.0, 1.0, 1.0)),
              ("gain 0.3, offset 30", 0.3, 30.0, (1.0, 1.0, 1.0)), ("gain 0.5, offset 20, cast (1, 0.9, 0.7)", 0.5, 20.0, (1.0, 0.9, 0.7))]


def use(a):
    m, pages = deck(a.pages)
    frames, truth, _ = synth.frames(pages, 32, W, H, threads=NCPU)
    truth = np.asarray(truth)
    shown = truth >= 0
    res = {"shape": "%d pages of 2001x1125, 32 1080p frames of which %d show a page, ORB-1000" % (a.pages, int(shown.sum())), "rows": []}
    for name, gain, offset, cast in DARKENINGS:
        dark = np.clip(frames.astype(np.float32) * gain * np.asarray(cast, np.float32) + offset, 0, 255).astype(np.uint8)
        row = {"frames": name}
        for tag in ("plain", "levels"):
            lo = hi = None
            if tag == "levels":
                m.levels_begin()
                m.observe_frames(dark)
                lo, hi = m.levels_points(0.01, 0.01)
                m.levels_end()
                m.set_frame_levels(_capi.frame_levels_lut(lo, hi))
            v = m.match_frames(dark)
            m.set_frame_levels(None)
            right = int((v["page_idx"][shown] == truth[shown]).sum())
            none = int((v["page_idx"][shown] < 0).sum())
            sim = v["similarity"][shown & (v["page_idx"] >= 0)]
            row[tag] = {"right": right, "none": none, "wrong": int(shown.sum()) - right - none,
                        "median_similarity": float(np.median(sim)) if len(sim) else None, "points": [lo, hi]}
            print("use: %-42s %-6s right %2d / %d  none %2d  median similarity %s  points %s" % (
                name, tag, right, int(shown.sum()), none, "%.3f" % np.median(sim) if len(sim) else "-", (lo, hi) if lo else ""), flush=True)
        res["rows"].append(row)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--hist", action="store_true")
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--content", default="noise", choices=["noise", "slide", "constant"])
    ap.add_argument("--pages", type=int, default=24)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    if a.hist:
        hist(a)
    if a.use:
        use(a)


if __name__ == "__main__":
    main()
