#!/usr/bin/env python3
"""Frame lens (include/slideo_amd.h "Frame lens"): the records of docs/EXTENSIONS.md.  One process per mode:

  --kernels   128 device-resident 1080p BGR frames through the observe call with a content session open, under five settings in
              alternated rounds (--rounds, default 3): the region's three own instances — a keystoned quad (rectify_kernel<0>), an
              affine map (rectify_kernel<1>), an integer shift by (4, 2) (rectify_kernel<2>) —, a lens alone (lens_kernel<false>) and
              the lens with the keystoned quad (lens_kernel<true>); every output 1920x1080.  Run it under a
              profiler's kernel trace with statistics, in a run of its own (python profiles/summarize_rocpd.py <results.db>); the wall
              time of every call is printed as well.
  --call      a headline-sized call (--frames 256 device-resident 1080p synthetic frames, --pages 100, ORB-1000) under the region alone
              and under lens plus region, alternated (--rounds, default 5): the step times, their medians and spread, one JSON line.

    python tools/frame_lens_rate.py --kernels [--content noise] | --call [--frames 256] [--pages 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, N = 1920, 1080, 128
QUAD = [(24.5, 16.25), (1896.0, 10.0), (1908.5, 1070.5), (12.0, 1064.5)]
K1 = -0.08


def lens():
    return (W, H, (W - 1) / 2.0, (H - 1) / 2.0, 0.5 * float(np.hypot(W, H)), K1, 0.0)


def kernels(a):
    import torch
    from slideo_amd import _capi, synth
    if a.content == "noise":
        d = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device="cuda")
    else:
        pages = synth.pages(2, 2001, 1125)
        frames, _, _ = synth.frames(pages, 2, W, H)
        d = torch.from_numpy(frames[1]).cuda()[None].expand(N, H, W, 3).contiguous()
    torch.cuda.synchronize()
    m = _capi.Matcher(_capi.default_config())
    settings = (("region, keystoned quad: rectify_kernel<0>", (W, H, QUAD, W, H), None),
                ("region, affine: rectify_kernel<1>", (W, H, [0.98, 0.01, 12.5, -0.01, 0.98, 9.25, 0, 0, 1.0], W, H), None),
                ("region, integer shift: rectify_kernel<2>", (W, H, [1, 0, 4, 0, 1, 2, 0, 0, 1], W, H), None),
                ("lens alone: lens_kernel<false>", None, lens()),
                ("lens + keystoned quad: lens_kernel<true>", (W, H, QUAD, W, H), lens()))
    m.content_begin(24)
    for rnd in range(a.rounds):
        for tag, region, ln in settings:
            m.clear_frame_lens(); m.clear_frame_region()
            if region is not None:
                m.set_frame_region(*region)
            if ln is not None:
                m.set_frame_lens(*ln)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.observe_frames_dev(d.data_ptr(), N, W, H)
            print("kernels %s: round %d: %s: observe call of %d frames %.1f ms" % (a.content, rnd, tag, N, (time.perf_counter() - t0) * 1e3), flush=True)
    m.content_end()
    m.close()


def call(a):
    import torch
    from slideo_amd import _capi, synth
    pages = synth.pages(a.pages, 2001, 1125)
    frames, truth, _ = synth.frames(pages, a.frames, W, H)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000), device=0)
    m.add_pages(list(pages)); m.finalize()
    t = torch.from_numpy(frames).cuda()
    m.set_frame_region(W, H, QUAD, W, H)
    ms = {"region": [], "lens + region": []}
    for rnd in range(a.rounds + 1):                                # (round 0 sizes the workspaces of both settings: not recorded)
        for tag, ln in (("region", None), ("lens + region", lens())):
            if ln is None:
                m.clear_frame_lens()
            else:
                m.set_frame_lens(*ln)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = m.match_frames_dev(t.data_ptr(), a.frames, W, H)
            dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                ms[tag].append(round(dt, 3))
    rec = dict(frames=a.frames, pages=a.pages, rounds=a.rounds, k1=K1, ms=ms, median={k: float(np.median(v_)) for k, v_ in ms.items()},
               spread={k: [min(v_), max(v_)] for k, v_ in ms.items()}, paged_last=int((v["page_idx"] >= 0).sum()))
    for k in ms:
        print("call of %d frames, %s: median %.3f ms, %.3f .. %.3f over %d alternated repeats" % (a.frames, k, rec["median"][k], *rec["spread"][k], a.rounds))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--call", action="store_true")
    ap.add_argument("--content", default="noise", choices=["noise", "slide"])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=0)
    a = ap.parse_args()
    if a.kernels:
        a.rounds = a.rounds or 3
        return kernels(a)
    a.rounds = a.rounds or 5
    return call(a)


if __name__ == "__main__":
    main()
