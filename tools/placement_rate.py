#!/usr/bin/env python3
"""Match placement map (include/slideo_amd.h "Match placement map"): the records of docs/EXTENSIONS.md "Match placement map".

usage: python tools/placement_rate.py [--frames 256] [--pages 100] [--kernels-only | --keystone]

Default: 1080p synthetic frames against a synthetic deck (ORB-1000) matched twice, without and with a placement session — the
verdict bytes must agree —, the wall time of both calls and the session's totals, one line each and a JSON line at the end.
--kernels-only: for a rocprofv3 --kernel-trace --stats run of its own — the device-resident frames matched three times under a
placement AND an evidence session, so that placement_kernel stands beside evidence_kernel (its yardstick: it walks the same votes)
and verdict_kernel in one trace (python profiles/summarize_rocpd.py <results.db>), and nothing else.
--keystone: the keystone scene of tests/placement_ref.py (960x540) — the learnt quad's corner error, and the share of frames
assigned to the truth without a region, with the learnt region and with the scene's true region."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def keystone():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import placement_ref as P
    from slideo_amd import _capi, matching, synth
    U = P.USE
    pages, frames, truth = P.keystone_scene(synth)
    m = _capi.Matcher(_capi.default_config(nfeatures=U["nfeatures"], min_rating=U["min_rating"]), device=0)
    m.add_pages(list(pages)); m.finalize()
    sw, sh, quad, ow, oh = matching.learn_frame_quad_from_matches(m, [frames], cell=U["cell"], min_inliers=U["min_inliers"], reach=U["reach"],
                                                                   min_count=U["min_count"], trim=U["trim"], rounds=U["rounds"])
    rec = dict(corner_error_px=round(P.corner_error(quad), 3), out=(ow, oh))

    def share(region):
        if region is not None:
            m.set_frame_region(sw, sh, region, ow, oh)
        try:
            v = m.match_frames(frames)
        finally:
            m.clear_frame_region()
        return float((v["page_idx"] == truth).mean()), float(v["inliers"].mean()), float(v["similarity"].mean())
    for name, region in (("none", None), ("learnt", quad), ("true", [tuple(c) for c in P.KEYSTONE_QUAD])):
        r, inl, sim = share(region)
        rec[name] = dict(right=round(r, 3), mean_inliers=round(inl, 2), mean_similarity=round(sim, 4))
        print("region %-6s: %.3f of %d frames right, mean winning inliers %.2f, mean similarity %.4f" % (name, r, len(frames), inl, sim))
    print("learnt quad %s, largest corner error %.3f px" % ([tuple(round(c, 2) for c in p) for p in quad], rec["corner_error_px"]))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--min-inliers", type=int, default=20)
    ap.add_argument("--reach", type=float, default=8.0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--keystone", action="store_true")
    a = ap.parse_args()
    if a.keystone:
        return keystone()
    import torch
    from slideo_amd import _capi, synth
    pages = synth.pages(a.pages, 2001, 1125)
    frames, truth, _ = synth.frames(pages, a.frames, 1920, 1080)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000), device=0)
    m.add_pages(list(pages)); m.finalize()
    t = torch.from_numpy(frames).cuda()
    call = lambda: m.match_frames_dev(t.data_ptr(), a.frames, 1920, 1080)
    call()                                                     # (workspaces sized)
    session = (a.cell, a.min_inliers, a.reach)
    if a.kernels_only:
        m.placement_begin(*session)
        m.evidence_begin(a.cell, a.min_inliers)
        for _ in range(3):
            call()
        m.evidence_end()
        m.placement_end()
        return

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter(); v = call(); return v, (time.perf_counter() - t0) * 1e3
    plain, ms_plain = min((timed() for _ in range(5)), key=lambda r: r[1])
    m.placement_begin(*session)
    got, ms_on = min((timed() for _ in range(5)), key=lambda r: r[1])
    sums, through, counted = m.placement_sums()
    m.placement_end()
    assert got.tobytes() == plain.tobytes(), "verdict bytes differ under a session"
    rec = dict(frames=a.frames, pages=a.pages, cell=a.cell, min_inliers=a.min_inliers, reach=a.reach, ms_plain=round(ms_plain, 3),
               ms_session=round(ms_on, 3), frames_through=through, frames_counted=counted, keypoints=int(sums[0].sum()),
               right=int((plain["page_idx"] == truth).sum()))
    print("call of %d frames: %.3f ms without a session, %.3f ms with one (best of 5 each)" % (a.frames, ms_plain, ms_on))
    print("session: %d through, %d counted over 5 calls; %d keypoints summed" % (through, counted, rec["keypoints"]))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
