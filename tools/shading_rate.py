#!/usr/bin/env python3
"""Frame shading and the match shading map (include/slideo_amd.h "Frame shading", "Match shading map"): the records of
docs/EXTENSIONS.md.  One process per mode:

  --kernels   128 device-resident 1080p BGR frames through the observe call with a content session open, three calls each under (a) a
              levels table alone — levels_kernel, the yardstick: the same bytes, the same thread shape —, (b) a gain field alone —
              shading_kernel<false> —, (c) both — shading_kernel<true>, and no levels_kernel.  All three out of place, out of the
              caller's memory into the staging.  --content noise | slide.  Run it under a profiler's kernel trace with statistics, in
              a run of its own (python profiles/summarize_rocpd.py <results.db>).
  --map       1080p synthetic frames against a synthetic deck (ORB-1000), device-resident, matched three times with a tone session
              and a shading session open: shading_map_kernel beside tone_kernel, its yardstick, in one trace.  For a kernel-trace run
              of its own.
  --call      the same frames matched without and with a shading session — the verdict bytes must agree —: the wall time of both
              calls (best of 5 each) and the session's totals, one line each and a JSON line at the end.

    python tools/shading_rate.py --kernels [--content noise] | --map | --call [--frames 256] [--pages 100] [--cell 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, N = 1920, 1080, 128


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
    lut = _capi.frame_levels_lut([34] * 3, [106] * 3)
    gw, gh = -(-W // a.cell), -(-H // a.cell)
    j, i = np.mgrid[0:gh + 1, 0:gw + 1].astype(np.float64)
    gains = np.rint(256 * (1.0 + 1.5 * (((i - gw / 2) / (gw / 2)) ** 2 + ((j - gh / 2) / (gh / 2)) ** 2) / 2)).astype(np.uint16)
    m.content_begin(24)
    for tag, field, table in (("levels alone", None, lut), ("shading alone", gains, None), ("shading + levels, one pass", gains, lut)):
        m.set_frame_levels(table)
        if field is None:
            m.set_frame_shading(gains=None)
        else:
            m.set_frame_shading(W, H, a.cell, field)
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.observe_frames_dev(d.data_ptr(), N, W, H)
            print("kernels %s: %s: observe call of %d frames %.1f ms" % (a.content, tag, N, (time.perf_counter() - t0) * 1e3), flush=True)
    m.content_end()
    m.close()


def scene(a):
    import torch
    from slideo_amd import _capi, synth
    pages = synth.pages(a.pages, 2001, 1125)
    frames, truth, _ = synth.frames(pages, a.frames, W, H)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000), device=0)
    m.add_pages(list(pages)); m.finalize()
    t = torch.from_numpy(frames).cuda()
    call = lambda: m.match_frames_dev(t.data_ptr(), a.frames, W, H)
    call()                                                     # (workspaces sized)
    return m, call, truth, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--map", action="store_true")
    ap.add_argument("--call", action="store_true")
    ap.add_argument("--content", default="noise", choices=["noise", "slide"])
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--min-inliers", type=int, default=20)
    ap.add_argument("--min-hits", type=int, default=20)
    ap.add_argument("--flat", type=int, default=255)
    a = ap.parse_args()
    if a.kernels:
        return kernels(a)
    import torch
    m, call, truth, keep = scene(a)
    session = (a.cell, a.min_inliers, a.min_hits, a.flat)
    if a.map:
        m.tone_begin(a.min_inliers, a.min_hits, a.flat)
        m.shading_begin(*session)
        for _ in range(3):
            call()
        m.shading_end(); m.tone_end()
        return

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter(); v = call(); return v, (time.perf_counter() - t0) * 1e3
    plain, ms_plain = min((timed() for _ in range(5)), key=lambda r: r[1])
    m.shading_begin(*session)
    got, ms_on = min((timed() for _ in range(5)), key=lambda r: r[1])
    sums, through, counted = m.shading_sums()
    m.shading_end()
    assert got.tobytes() == plain.tobytes(), "verdict bytes differ under a session"
    rec = dict(frames=a.frames, pages=a.pages, cell=a.cell, min_inliers=a.min_inliers, min_hits=a.min_hits, flat=a.flat, ms_plain=round(ms_plain, 3),
               ms_session=round(ms_on, 3), frames_through=through, frames_counted=counted, samples=int(sums[0].sum()),
               cells_hit=int((sums[0] > 0).sum()), cells=int(sums[0].size), right=int((plain["page_idx"] == truth).sum()))
    print("call of %d frames: %.3f ms without a session, %.3f ms with one (best of 5 each)" % (a.frames, ms_plain, ms_on))
    print("session: %d through, %d counted over 5 calls; %d samples in %d of %d cells" % (through, counted, rec["samples"], rec["cells_hit"], rec["cells"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
