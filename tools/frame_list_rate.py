"""Cost of frame lists (include/slideo_amd.h "Frame lists").  One process per mode:

  --kernels   128 1080p frames, every plane its own device allocation, through the mask call of a DEVICE list (gather, conversion,
              small images; no pages needed), three times each as NV12, I420 and BGR8 — and, the yardstick in the same run, a
              device-to-device copy of the same bytes (one hipMemcpyAsync, timed with events and printed; under a profiler's memory-copy
              trace it is a row of its own).  Run it under a profiler's kernel trace with statistics, in a run of its own: the
              frame_gather_kernel rows are the time per 128 frames.  The expectation to report against is the copy's rate.
  --rates     host-fed match calls from PINNED memory, --frames 1080p frames against --pages pages, ORB-1000, NV12 and BGR8: the
              list call over frames in separate allocations against the contiguous call PLUS the host-side copy of those frames
              into one batch buffer that it needs; both legs in this process, alternated.
  --device    device-resident frames through submit / collect in units of --frames frames, --units units per repeat: the list
              (gathered) against contiguous device frames, NV12 (the price of the gather) and BGR8 (the price of the gather and of
              losing the in-place read), alternated.

    python tools/frame_list_rate.py --kernels | --rates | --device   [--frames 128] [--pages 100] [--reps 5] [--units 8]

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
from yuv_desc_rate import deck, W, H, NCPU  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def planes_of(frame, fmt):
    """The planes of one tight 1080p frame as 2-D byte views, and frame_list's `chroma` argument."""
    if fmt == "bgr":
        return [frame.reshape(H, W * 3)], None
    y = frame[: W * H].reshape(H, W)
    if fmt == "nv12":
        return [y, frame[W * H:].reshape(H // 2, W)], "uv"
    q = W * H // 4
    return [y, frame[W * H: W * H + q].reshape(H // 2, W // 2), frame[W * H + q:].reshape(H // 2, W // 2)], None


def separate(frames, fmt, where):
    """Every plane of every frame in an allocation of its own: where 'device', 'pinned' -> (FrameList, the tensors)."""
    out, keep = [], []
    for f in frames:
        pl, chroma = planes_of(f, fmt)
        ts = []
        for p in pl:
            t = torch.empty(p.shape, dtype=torch.uint8, device="cuda") if where == "device" else torch.empty(p.shape, dtype=torch.uint8, pin_memory=True)
            t.copy_(torch.from_numpy(np.ascontiguousarray(p)))
            ts.append(t)
        keep.append(ts)
        out.append(tuple(ts) if len(ts) > 1 else ts[0])
    torch.cuda.synchronize()
    return _capi.frame_list(out, "bgr" if fmt == "bgr" else "yuv", W, H, chroma=chroma), keep


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    for fmt, fb in (("nv12", W * H * 3 // 2), ("i420", W * H * 3 // 2), ("bgr", W * H * 3)):
        buf = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        fl, keep = separate(buf, fmt, "device")
        for _ in range(3):
            t0 = time.perf_counter()
            m.changed_mask_list(fl)
            print("kernels: %-5s mask call of a device list of %d frames %.1f ms" % (fmt, n, (time.perf_counter() - t0) * 1e3), flush=True)
        src = torch.from_numpy(buf).cuda()
        dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3
            print("kernels: %-5s device-to-device copy of the same %d bytes %.1f us = %.0f GB/s read + write" % (fmt, buf.size, us, 2 * buf.size / us / 1e3), flush=True)
        del fl, keep, src, dst
    m.close()


def _alternate(runs, reps, frames, res, tag):
    t = {k: [] for k in runs}
    for fn in runs.values():
        fn()
    for _ in range(reps):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    for k, v in t.items():
        r = mmm(v)
        res[k] = dict(r, frames_per_s=frames / (r["median"] * 1e-3))
        print("%s: %-22s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (tag, k, r["min"], r["median"], r["max"], frames,
                                                                                          res[k]["frames_per_s"]), flush=True)


def _encode(frames, fmt):
    import yuv420_ref
    n = len(frames)
    if fmt == "bgr":
        return np.ascontiguousarray(frames).reshape(n, -1)
    L, fb = _capi.yuv420_layout(fmt, W, H)
    return yuv420_ref.frames_to_yuv(frames, L, fb)


def rates(a):
    res = {"shape": "%d pages, %d 1080p frames from pinned memory, ORB-1000" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    idx = np.arange(a.frames) % 32
    runs, keep = {}, []
    for fmt in ("nv12", "bgr"):
        enc = _encode(frames, fmt)[idx]
        fl, k = separate(enc, fmt, "pinned")
        batch = torch.empty(enc.shape, dtype=torch.uint8, pin_memory=True)
        bnp = batch.numpy()
        srcs = [[t.numpy() for t in ts] for ts in k]
        keep += [fl, k, batch]
        L = _capi.yuv420_layout(fmt, W, H)[0] if fmt != "bgr" else None

        def contiguous(bnp=bnp, srcs=srcs, fmt=fmt, L=L):
            for i, pl in enumerate(srcs):                         # the copy an integration makes today: every plane into the batch
                o = 0
                for p in pl:
                    bnp[i, o: o + p.size] = p.reshape(-1)
                    o += p.size
            if fmt == "bgr":
                return m.match_frames(bnp.reshape(-1, H, W, 3))
            return m.match_frames_yuv420(bnp, W, H, L)
        want = contiguous()
        assert m.match_frames_list(fl).tobytes() == want.tobytes()
        runs["%s list" % fmt] = lambda fl=fl: m.match_frames_list(fl)
        runs["%s copy + contiguous" % fmt] = contiguous
    _alternate(runs, a.reps, a.frames, res, "rates")
    m.close()
    print(json.dumps(res))


def device(a):
    res = {"shape": "%d pages, device-resident 1080p frames, %d units of %d frames per repeat through submit / collect, ORB-1000" % (a.pages, a.units, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)
    idx = np.arange(a.frames) % 32
    runs, keep = {}, []

    def stream(submit):
        pend = []
        for _ in range(a.units):
            if len(pend) == m.max_in_flight():
                m.collect(pend.pop(0))
            pend.append(submit())
        return [m.collect(t) for t in pend]

    for fmt in ("nv12", "bgr"):
        enc = _encode(frames, fmt)[idx]
        fl, k = separate(enc, fmt, "device")
        d = torch.from_numpy(enc).cuda()
        keep += [fl, k, d]
        if fmt == "bgr":
            sub = lambda d=d: m.submit_dev(d.data_ptr(), a.frames, W, H)
        else:
            L, fb = _capi.yuv420_layout(fmt, W, H)
            sub = lambda d=d, L=L, fb=fb: m.submit_yuv420_dev(d.data_ptr(), a.frames, W, H, L, fb)
        runs["%s list" % fmt] = lambda fl=fl: stream(lambda: m.submit_list(fl))
        runs["%s contiguous" % fmt] = lambda sub=sub: stream(sub)
        assert runs["%s list" % fmt]()[-1].tobytes() == runs["%s contiguous" % fmt]()[-1].tobytes()
    _alternate(runs, a.reps, a.frames * a.units, res, "device")
    m.close()
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--units", type=int, default=8)
    a = ap.parse_args()
    (kernels if a.kernels else device if a.device else rates)(a)
