"""Frame rate of the working-size front door (include/slideo_amd.h "Working size") at the headline content (500 pages, ORB-1000),
in one process, alternated repeats:

  device-resident 4K BGR frames   (a) no working size   (b) working size 1920x1080   (c) the same content at native 1080p
  pinned host frames, 4K          BGR and NV12, (a) and (b)

and the share of frames assigned to the synthetic truth in (a), (b), (c).

    python tools/working_size_rate.py [--reps 3] [--frames 64] [--kernels-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: one call per reduce kernel and one 4K NV12 call (a
short run to trace reduce*_kernel beside yuv420_to_bgr_desc_kernel under rocprofv3 --kernel-trace --stats; a launch covers --frames
frames)."""
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
WS = (1920, 1080)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    B = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    f4k, truth, _ = synth.frames(pages, B, 3840, 2160, threads=NCPU)
    f1080, truth1080, _ = synth.frames(pages, B, 1920, 1080, threads=NCPU)      # the same stream (seed, pages, poses) at 1080p
    assert np.array_equal(truth, truth1080)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    L, fb = _capi.yuv420_layout("nv12", 3840, 2160)
    nh = min(B, 32)                                                             # frames of the host measurements
    nv12 = yuv420_ref.frames_to_yuv(f4k[:nh], L, fb)
    d4k = torch.from_numpy(f4k).cuda()
    d1080 = torch.from_numpy(f1080).cuda()
    dnv = torch.from_numpy(nv12).cuda()
    res = {"shape": "%d pages, %d frames, ORB-1000; 4K = 3840x2160, working size %dx%d" % (a.pages, B, WS[0], WS[1])}

    def dev(ptr, w, h, ws):
        m.set_working_size(*ws)
        return m.match_frames_dev(ptr, B, w, h)

    if a.kernels_only:
        fq, _, _ = synth.frames(pages, B, 2560, 1440, threads=NCPU)
        f3, _, _ = synth.frames(pages, B, 2880, 1620, threads=NCPU)
        dq, d3 = torch.from_numpy(fq).cuda(), torch.from_numpy(f3).cuda()
        for _ in range(2):
            dev(d4k.data_ptr(), 3840, 2160, WS)                                  # reduce2x2_kernel
            dev(dq.data_ptr(), 2560, 1440, WS)                                   # reduce_area_kernel (4/3)
            dev(d3.data_ptr(), 2880, 1620, (960, 540))                           # reduce_int_kernel (factor 3)
            m.set_working_size(*WS)
            m.match_frames_yuv420_dev(dnv.data_ptr(), nh, 3840, 2160, L, fb)     # yuv420_to_bgr_desc_kernel at 4K, then reduce2x2_kernel
        m.close()
        return

    runs = {"a_4k": lambda: dev(d4k.data_ptr(), 3840, 2160, (0, 0)), "b_4k_ws": lambda: dev(d4k.data_ptr(), 3840, 2160, WS),
            "c_1080": lambda: dev(d1080.data_ptr(), 1920, 1080, (0, 0))}
    for fn in runs.values():
        fn()                                                                    # (warm: workspaces sized, tables built)
    t = {k: [] for k in runs}
    acc = {}
    for _ in range(a.reps):                                                     # (alternating, so that clock and thermal drift hit all alike)
        for k, fn in runs.items():
            dt, v = timed(fn)
            t[k].append(dt)
            acc[k] = float((v["page_idx"] == truth).mean())
    for k in runs:
        med = float(np.median(t[k]))
        res["device_%s_ms" % k] = [x * 1e3 for x in t[k]]
        res["device_%s_fps" % k] = B / med
        res["truth_share_%s" % k] = acc[k]
        print("device %-8s %s ms (median %.2f) = %.0f frames/s | assigned to the truth %.3f"
              % (k, " ".join("%.2f" % (x * 1e3) for x in t[k]), med * 1e3, B / med, acc[k]), flush=True)
    ma, mb, mc = (float(np.median(t[k])) for k in ("a_4k", "b_4k_ws", "c_1080"))
    res["device_b_over_a"] = ma / mb
    res["device_b_over_c"] = mc / mb
    res["device_b_minus_c_ms"] = (mb - mc) * 1e3
    res["device_c_spread_ms"] = (max(t["c_1080"]) - min(t["c_1080"])) * 1e3
    print("device (b)/(a) %.2fx  (b)/(c) %.3fx  (b) - (c) %.2f ms per %d frames  spread of (c) %.2f ms"
          % (ma / mb, mc / mb, (mb - mc) * 1e3, B, res["device_c_spread_ms"]), flush=True)

    pin_bgr = torch.from_numpy(f4k[:nh]).pin_memory().numpy()
    pin_nv = torch.from_numpy(nv12).pin_memory().numpy()

    def host(kind, ws):
        m.set_working_size(*ws)
        return m.match_frames(pin_bgr) if kind == "bgr" else m.match_frames_yuv420(pin_nv, 3840, 2160, L)
    hruns = {(k, n): (lambda k=k, ws=ws: host(k, ws)) for k in ("bgr", "nv12") for n, ws in (("a", (0, 0)), ("b", WS))}
    for fn in hruns.values():
        fn()
    ht = {k: [] for k in hruns}
    for _ in range(a.reps):
        for k, fn in hruns.items():
            ht[k].append(timed(fn)[0])
    for (k, n), ts in ht.items():
        med = float(np.median(ts))
        res["host_pinned_%s_%s_fps" % (k, n)] = nh / med
        print("host pinned 4K %-4s (%s) %s ms = %.0f frames/s" % (k, n, " ".join("%.2f" % (x * 1e3) for x in ts), nh / med), flush=True)
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
