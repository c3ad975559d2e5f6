#!/usr/bin/env python3
"""Match tone table (include/slideo_amd.h "Match tone table"): the records of docs/EXTENSIONS.md "Match tone table".

usage: python tools/tone_rate.py [--frames 256] [--pages 100] [--flat 255] [--kernels-only]

Default: 1080p synthetic frames against a synthetic deck (ORB-1000) matched twice, without and with a tone session — the verdict
bytes must agree —, the wall time of both calls and the session's totals, one line each and a JSON line at the end.
--kernels-only: for a rocprofv3 --kernel-trace --stats run of its own — the device-resident frames matched three times under a
session, so that tone_kernel stands beside reproject_vt_kernel (its yardstick), verdict_kernel and the unit's copies in one trace
(python profiles/summarize_rocpd.py <results.db>), and nothing else."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--min-inliers", type=int, default=20)
    ap.add_argument("--min-hits", type=int, default=20)
    ap.add_argument("--flat", type=int, default=255)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch
    from slideo_amd import _capi, synth
    pages = synth.pages(a.pages, 2001, 1125)
    frames, truth, _ = synth.frames(pages, a.frames, 1920, 1080)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000), device=0)
    m.add_pages(list(pages)); m.finalize()
    t = torch.from_numpy(frames).cuda()
    call = lambda: m.match_frames_dev(t.data_ptr(), a.frames, 1920, 1080)
    call()                                                     # (workspaces sized)
    session = (a.min_inliers, a.min_hits, a.flat)
    if a.kernels_only:
        m.tone_begin(*session)
        for _ in range(3):
            call()
        m.tone_end()
        return

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter(); v = call(); return v, (time.perf_counter() - t0) * 1e3
    plain, ms_plain = min((timed() for _ in range(5)), key=lambda r: r[1])
    m.tone_begin(*session)
    got, ms_on = min((timed() for _ in range(5)), key=lambda r: r[1])
    cnt, sm, through, counted = m.tone_counts()
    m.tone_end()
    assert got.tobytes() == plain.tobytes(), "verdict bytes differ under a session"
    rec = dict(frames=a.frames, pages=a.pages, min_inliers=a.min_inliers, min_hits=a.min_hits, flat=a.flat, ms_plain=round(ms_plain, 3),
               ms_session=round(ms_on, 3), frames_through=through, frames_counted=counted, samples=int(cnt[0].sum()),
               right=int((plain["page_idx"] == truth).sum()))
    print("call of %d frames: %.3f ms without a session, %.3f ms with one (best of 5 each)" % (a.frames, ms_plain, ms_on))
    print("session: %d through, %d counted over 5 calls; %d samples per channel" % (through, counted, rec["samples"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
