"""Cost of the frame pixel format (include/slideo_amd.h "Frame pixel format").  One process per mode:

  --kernels   128 1080p frames through the mask call (upload, conversion out of device memory, small images; no pages needed),
              three times under each of RGB8, BGRA8 and PLANAR_RGB8 — the three instances of pixels_to_bgr_kernel — and, the
              yardstick in the same run, I444 under the YUV sampling 444: yuv_sampled_to_bgr_kernel<444, 8> moves the same 3 + 3
              bytes per pixel with the same thread shape.  Run it under a profiler's kernel trace with statistics, in a run of its
              own: the *_to_bgr rows are the time per 128 frames of each kernel.  It prints nothing but the wall times.
  --rates     host-fed match calls from PINNED memory, --frames 1080p frames against --pages pages, ORB-1000: BGR, RGB, BGRA and
              planar RGB of the same frames, alternated, min / median / max.
  --device    device-resident frames through submit / collect in units of --frames frames, --units units per repeat: RGB (converted
              out of the caller's memory) against BGR (read in place), alternated: the cost of losing the in-place read.

    python tools/pixel_format_rate.py --kernels | --rates | --device   [--frames 128] [--pages 100] [--reps 5] [--units 8]

Prints one line per measurement and a JSON line at the end."""
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
from direct_rate import mmm  # noqa: E402
from yuv_desc_rate import deck, pinned, W, H, NCPU  # noqa: E402


def encode(frames, fmt):
    """[n, H, W, 3] BGR -> the same frames in the array shape of `fmt` ('bgr', 'rgb', 'bgra', 'planar_rgb'), tight."""
    if fmt == "bgr":
        return np.ascontiguousarray(frames)
    if fmt == "rgb":
        return np.ascontiguousarray(frames[..., ::-1])
    if fmt == "bgra":
        return np.ascontiguousarray(np.concatenate([frames, np.full(frames.shape[:3] + (1,), 255, np.uint8)], axis=3))
    if fmt == "planar_rgb":
        return np.ascontiguousarray(frames[..., ::-1].transpose(0, 3, 1, 2))
    raise ValueError(fmt)


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    for fmt, shape in (("rgb", (n, H, W, 3)), ("bgra", (n, H, W, 4)), ("planar_rgb", (n, 3, H, W))):
        buf = rng.integers(0, 256, shape, dtype=np.uint8)
        m.set_pixel_format(fmt)
        for _ in range(3):
            t0 = time.perf_counter()
            m.changed_mask(buf)
            print("kernels: %-10s mask call of %d frames %.1f ms" % (fmt, n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.set_pixel_format("bgr")
    L, fb = _capi.yuv_layout("i444", W, H)
    buf = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    m.set_yuv_sampling("444")
    for _ in range(3):
        t0 = time.perf_counter()
        m.changed_mask_yuv420(buf, W, H, L)
        print("kernels: %-10s mask call of %d frames %.1f ms" % ("i444", n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.close()


def _alternate(runs, reps, frames, res, tag):
    t = {k: [] for k in runs}
    for prep, fn in runs.values():
        prep()
        fn()
    for _ in range(reps):
        for k, (prep, fn) in runs.items():
            prep()
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    for k, v in t.items():
        r = mmm(v)
        res[k] = dict(r, frames_per_s=frames / (r["median"] * 1e-3))
        print("%s: %-10s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (tag, k, r["min"], r["median"], r["max"], frames,
                                                                                          res[k]["frames_per_s"]), flush=True)


def rates(a):
    res = {"shape": "%d pages, %d 1080p frames from pinned memory, ORB-1000" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    idx = np.arange(a.frames) % 32
    runs = {}
    for fmt in ("bgr", "rgb", "bgra", "planar_rgb"):
        enc = encode(frames, fmt)[idx]
        buf = pinned(enc.reshape(a.frames, -1))
        runs[fmt] = (lambda fmt=fmt: m.set_pixel_format(fmt), lambda buf=buf, shape=enc.shape: m.match_frames(buf.numpy().reshape(shape)))
    _alternate(runs, a.reps, a.frames, res, "rates")
    m.close()
    print(json.dumps(res))


def device(a):
    res = {"shape": "%d pages, device-resident 1080p frames, %d units of %d frames per repeat through submit / collect, ORB-1000" % (a.pages, a.units, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)
    idx = np.arange(a.frames) % 32
    runs = {}
    keep = []
    for fmt in ("bgr", "rgb"):
        d = torch.from_numpy(encode(frames, fmt)[idx]).cuda()
        keep.append(d)

        def run(d=d):
            pend = []
            for _ in range(a.units):
                if len(pend) == m.max_in_flight():
                    m.collect(pend.pop(0))
                pend.append(m.submit_dev(d.data_ptr(), a.frames, W, H))
            for t in pend:
                m.collect(t)
        runs[fmt] = (lambda fmt=fmt: m.set_pixel_format(fmt), run)
    torch.cuda.synchronize()
    _alternate(runs, a.reps, a.frames * a.units, res, "device")
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--units", type=int, default=8)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    if a.rates:
        rates(a)
    if a.device:
        device(a)


if __name__ == "__main__":
    main()
