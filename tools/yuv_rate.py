"""Frame rate of the YUV 4:2:0 front door against BGR at the headline shape (500 pages, 256 x 1080p, ORB-1000), in one process:
the host entry point (pageable and pinned sources) for BGR and NV12, and the device-resident path through submit / collect.

    python tools/yuv_rate.py [--reps 3] [--device-only]

Prints one line per measurement and a JSON line at the end.  --device-only skips the host calls (a short run to trace
yuv420_to_bgr_desc_kernel under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

from slideo_amd import _capi, synth  # noqa: E402
import yuv420_ref  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)


def timed(fn, reps):
    fn()                                                       # (warm: workspaces sized, tables built)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def stream(m, submit, n, unit):
    """n frames through submit / collect in units, up to max_in_flight at once (the steady state of a caller that keeps the GPU fed)."""
    pend = []
    for i in range(0, n, unit):
        if len(pend) == m.max_in_flight():
            m.collect(pend.pop(0))
        pend.append(submit(i, min(unit, n - i)))
    for t in pend:
        m.collect(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    B, w, h = 256, 1920, 1080
    pages = synth.pages(500, 2001, 1125, threads=NCPU)
    frames, _, _ = synth.frames(pages, B, w, h, threads=NCPU)
    L, fb = _capi.yuv420_layout("nv12", w, h)
    nv12 = yuv420_ref.frames_to_yuv(frames, L, fb)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, 500, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    res = {"shape": "500 pages, %d x %dx%d, ORB-1000" % (B, w, h), "bgr_bytes_per_frame": w * h * 3, "nv12_bytes_per_frame": fb}
    if not a.device_only:
        pin_bgr = torch.from_numpy(frames).pin_memory().numpy()
        pin_nv12 = torch.from_numpy(nv12).pin_memory().numpy()
        for name, bgr, yuv in (("pageable", frames, nv12), ("pinned", pin_bgr, pin_nv12)):
            tb = timed(lambda: m.match_frames(bgr), a.reps)
            ty = timed(lambda: m.match_frames_yuv420(yuv, w, h, L), a.reps)
            res["host_%s_bgr_fps" % name] = B / tb
            res["host_%s_nv12_fps" % name] = B / ty
            res["host_%s_nv12_over_bgr" % name] = tb / ty
            print("host %-8s BGR %.1f ms = %.0f frames/s | NV12 %.1f ms = %.0f frames/s | NV12 / BGR %.2fx"
                  % (name, tb * 1e3, B / tb, ty * 1e3, B / ty, tb / ty), flush=True)
    d_bgr = torch.from_numpy(frames).cuda()
    d_nv12 = torch.from_numpy(nv12).cuda()
    unit = B // 2
    fsb = w * h * 3

    def dev_bgr():
        stream(m, lambda i, k: m.submit_dev(d_bgr.data_ptr() + i * fsb, k, w, h), B, unit)

    def dev_nv12():
        stream(m, lambda i, k: m.submit_yuv420_dev(d_nv12.data_ptr() + i * fb, k, w, h, L, fb), B, unit)
    # (alternating, so that clock and thermal drift hit both alike)
    tb, ty = [], []
    for _ in range(a.reps):
        tb.append(timed(dev_bgr, 1))
        ty.append(timed(dev_nv12, 1))
    tb, ty = float(np.median(tb)), float(np.median(ty))
    res["device_bgr_fps"] = B / tb
    res["device_nv12_fps"] = B / ty
    res["device_nv12_over_bgr"] = tb / ty
    print("device   BGR %.1f ms = %.0f frames/s | NV12 %.1f ms = %.0f frames/s | NV12 / BGR %.3fx"
          % (tb * 1e3, B / tb, ty * 1e3, B / ty, tb / ty), flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
