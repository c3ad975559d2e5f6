"""Cost and use of the frame activity map (include/slideo_amd.h "Frame activity map").  One process, alternated repeats,
min / median / max:

  rate   observe_frames over 1080p frames — pinned host BGR, pinned host NV12, device-resident BGR — against slideo_changed_mask_*
         on the same host frames: the existing call that stages every frame and does little else
  use    the stream of tools/gate_mask_rate.py (500 pages, ORB-1000, 256 device-resident 1080p frames, holds of geometric length, the
         speaker-sized inset re-randomised on every frame): the mask learnt from it (--delta, --max-share, --grow) against that tool's
         hand-made hole — n_masked and the pixels that differ — and the gated stream's rate under either; the same with the inset as
         the held content +- A grey levels for each A of --amplitudes (where does delta stop separating?)

    python tools/activity_rate.py [--frames 256] [--pages 500] [--reps 5] [--delta 24] [--max-share 0.5] [--grow 1]
                                  [--amplitudes 10,40,80] [--rate-only] [--kernels-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: for a rocprofv3 --kernel-trace --stats run of its own —
128 device-resident 1080p frames observed as BGR (activity_kernel alone), as NV12 (yuv420_to_bgr_desc_kernel in front) and 128 4K frames
under a 1920x1080 working size (reduce2x2_kernel in front), three times each and nothing else."""
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

W, H = 1920, 1080
UNIT = 128


def mmm(ts):
    ms = sorted(x * 1e3 for x in ts)
    return {"min": ms[0], "median": float(np.median(ms)), "max": ms[-1]}


def timed(runs, reps):
    for fn in runs.values():
        fn()                                                                    # (warm: buffers sized)
    t = {k: [] for k in runs}
    for _ in range(reps):                                                       # (alternating, so that clock and thermal drift hit all alike)
        for k, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return {k: mmm(v) for k, v in t.items()}


def report(name, r, n):
    print("%-34s min %.2f median %.2f max %.2f ms per %d frames = %.0f frames/s" % (name, r["min"], r["median"], r["max"], n, n / (r["median"] * 1e-3)),
          flush=True)


def noisy_frames(n, gen):
    """n device-resident 1080p frames: a still image with a little noise on every frame (the content does not change the cost)."""
    base = torch.randint(0, 256, (1, H, W, 3), device="cuda", generator=gen, dtype=torch.uint8)
    d = base.repeat(n, 1, 1, 1)
    d[:, 700:, 1200:] = torch.randint(0, 256, (n, H - 700, W - 1200, 3), device="cuda", generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize()                      # (the library's streams do not wait for torch's: hip_stream is not passed below)
    return d


def observe(m, fn, delta):
    m.activity_begin(delta)
    fn()


def kernels_only(a):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261018)
    n = 128
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    d = noisy_frames(n, gen)
    L, fb = _capi.yuv420_layout("nv12", W, H)
    y = torch.randint(16, 236, (n, fb), device="cuda", generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize()
    for _ in range(3):
        observe(m, lambda: m.observe_frames_dev(d.data_ptr(), n, W, H), a.delta)
        observe(m, lambda: m.observe_frames_yuv420_dev(y.data_ptr(), n, W, H, L, fb), a.delta)
    del d, y
    big = torch.randint(0, 256, (n, 2 * H, 2 * W, 3), device="cuda", generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize()
    m.set_working_size(W, H)
    for _ in range(3):
        observe(m, lambda: m.observe_frames_dev(big.data_ptr(), n, 2 * W, 2 * H), a.delta)
    assert m.activity_info()["aw"] == W and m.activity_info()["pairs"] == n - 1
    m.activity_end()
    m.close()


def rate(a, res):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261018)
    n = a.frames
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    d = noisy_frames(n, gen)
    pin = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
    pin.copy_(d)
    host = pin.numpy()
    L, fb = _capi.yuv420_layout("nv12", W, H)
    ypin = torch.empty((n, fb), dtype=torch.uint8, pin_memory=True)
    ypin.copy_(torch.randint(16, 236, (n, fb), device="cuda", generator=gen, dtype=torch.uint8))
    yhost = ypin.numpy()
    r = timed({"observe_host_bgr_pinned": lambda: observe(m, lambda: m.observe_frames(host), a.delta),
               "changed_mask_host_bgr_pinned": lambda: m.changed_mask(host),
               "observe_host_nv12_pinned": lambda: observe(m, lambda: m.observe_frames_yuv420(yhost, W, H, L), a.delta),
               "changed_mask_host_nv12_pinned": lambda: m.changed_mask_yuv420(yhost, W, H, L),
               "observe_device_bgr": lambda: observe(m, lambda: m.observe_frames_dev(d.data_ptr(), n, W, H), a.delta)}, a.reps)
    for k, v in r.items():
        report("rate: " + k, v, n)
    res["rate_ms"] = r
    m.activity_end()
    m.close()


def use(a, res):
    from changed_gate_rate import lecture, stream
    from frame_mask_rate import inset_rect
    ncpu = min(16, os.cpu_count() or 1)
    n = a.frames
    pages = synth.pages(a.pages, 2001, 1125, threads=ncpu)
    seq = lecture(pages, n, a.share)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    y0, x0 = inset_rect(W, H)
    hole = np.full((H, W), 255, np.uint8)
    hole[y0:, x0:] = 0
    d_clean = torch.from_numpy(seq).cuda()
    fbb = W * H * 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261017)
    ih, iw = H - y0, W - x0
    BOTH = _capi.MASK_DETECT | _capi.MASK_GATE
    m.set_frame_mask_scope(BOTH)

    def with_inset(amplitude):
        d = d_clean.clone()
        if amplitude is None:
            d[:, y0:, x0:] = torch.randint(0, 2, (n, ih, iw, 1), device="cuda", generator=gen, dtype=torch.uint8) * 255
        else:
            noise = torch.randint(-amplitude, amplitude + 1, (n, ih, iw, 3), device="cuda", generator=gen, dtype=torch.int16)
            d[:, y0:, x0:] = (d[:, y0:, x0:].to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
        torch.cuda.synchronize()                  # (the frames are observed on the library's stream next)
        return d

    def gated(d):
        m.gate_reset(None)
        out = []
        stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fbb, c, W, H), lambda t: out.append(m.collect_changed(t)), n, UNIT)
        return np.concatenate([o[0] for o in out])

    def learn(d):
        m.activity_begin(a.delta)
        m.observe_frames_dev(d.data_ptr(), n, W, H)
        out = m.activity_mask(a.max_share, a.grow)
        m.activity_end()
        return out

    m.set_frame_mask(hole)
    clean_flags = gated(d_clean)
    res["use"] = {"hole_n_masked": int((hole == 0).sum()), "clean_changed_share": float(clean_flags.mean()),
                  "delta": a.delta, "max_share": a.max_share, "grow": a.grow}
    for amp in [None] + [int(x) for x in a.amplitudes.split(",") if x]:
        name = "texture" if amp is None else "pm%d" % amp
        d = with_inset(amp)
        mask, na, nm = learn(d)
        differ = int((mask != hole).sum())
        u = {"n_active": na, "n_masked": nm, "pixels_differ_from_hole": differ, "masked_outside_hole": int(((mask == 0) & (hole != 0)).sum()),
             "unmasked_inside_hole": int(((mask != 0) & (hole == 0)).sum())}
        m.set_frame_mask(hole)
        f_hole = gated(d)
        u["changed_share_hole"] = float(f_hole.mean())
        if nm < W * H:
            try:
                m.set_frame_mask(mask)
                f_learnt = gated(d)
                u["changed_share_learnt"] = float(f_learnt.mean())
                u["learnt_flags_equal_clean"] = bool(np.array_equal(f_learnt, clean_flags))
            except _capi.SlideoError as e:
                u["learnt_refused"] = str(e)
        print("inset %-8s learnt: n_active %d n_masked %d (hole %d), %d pixels differ (%d outside, %d inside); changed share hole %.3f learnt %s"
              % (name, na, nm, res["use"]["hole_n_masked"], differ, u["masked_outside_hole"], u["unmasked_inside_hole"], u["changed_share_hole"],
                 u.get("changed_share_learnt")), flush=True)
        if amp is None and "changed_share_learnt" in u:
            t = {"gated_hole": [], "gated_learnt": []}
            for rep in range(a.reps + 1):                                       # (rep 0 warms; the set call stays outside the timed interval)
                for k, msk in (("gated_hole", hole), ("gated_learnt", mask)):
                    m.set_frame_mask(msk)
                    t0 = time.perf_counter()
                    gated(d)
                    if rep:
                        t[k].append(time.perf_counter() - t0)
            u["ms"] = {k: mmm(v) for k, v in t.items()}
            for k, v in u["ms"].items():
                report("use: " + k, v, n)
            lt = timed({"learn": lambda: learn(d)}, a.reps)["learn"]
            report("use: learn (begin, observe, mask, end)", lt, n)
            u["learn_ms"] = lt
        res["use"][name] = u
        del d
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--delta", type=int, default=24)
    ap.add_argument("--max-share", type=float, default=0.5)
    ap.add_argument("--grow", type=int, default=1)
    ap.add_argument("--amplitudes", default="10,40,80")
    ap.add_argument("--rate-only", action="store_true")
    ap.add_argument("--use-only", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a)
        return
    res = {"shape": "%d 1080p frames" % a.frames}
    if not a.use_only:
        rate(a, res)
    if not a.rate_only:
        use(a, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
