"""Cost and use of the frame content box (include/slideo_amd.h "Frame content box").  One process, alternated repeats,
min / median / max:

  rate   observe_frames over 1080p frames — pinned host BGR, pinned host NV12, device-resident BGR — with an activity session only,
         a content session only and both open: does one pass with both cost less than two passes?
  use    a synthetic SCREEN RECORDING in the manner of tools/direct_rate.py, the pages 4:3 (1440x1080) and pillarboxed in 1080p
         frames: holds of geometric length (mean 1 / --share) show a deck page plus noise of +- --noise grey levels or — a share
         --moved of the holds — one of the generator's transformed frames; the bars are noise in 0..--level.  The region learnt
         from the frames (--level, --min-share, --min-fill) against the pasted box; the gated stream (submit / collect, units of
         128, direct similarity --t) without a region and with the learnt one: the share of changed frames resolved directly and
         the time per stream; the time of learning (begin, observe, box, end)

    python tools/content_box_rate.py [--frames 256] [--pages 500] [--reps 5] [--level 32] [--min-share 0.5] [--min-fill 0.25]
                                     [--share 0.5] [--moved 0.25] [--noise 3] [--t 0.9] [--rate-only] [--use-only] [--kernels-only]

Prints one line per measurement and a JSON line at the end.  --kernels-only: for a rocprofv3 --kernel-trace --stats run of its own —
128 device-resident 1080p frames observed as BGR with an activity session only, a content session only and both (activity_kernel and
content_kernel on the same frames), as NV12 with both open (yuv420_to_bgr_desc_kernel in front) and 128 4K frames under a 1920x1080
working size with both open (reduce2x2_kernel in front), three times each, then the box read out three times (content_fill_kernel),
and nothing else."""
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
from activity_rate import mmm, noisy_frames, report, timed  # noqa: E402

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
PW, PH = 1440, 1080                  # a 4:3 page at the frame's height
X0 = (W - PW) // 2
UNIT = 128
DELTA = 24


def observe(m, fn, a, activity, content):
    """One pass of fn over fresh sessions: activity, content or both"""
    m.activity_end(); m.content_end()
    if activity:
        m.activity_begin(DELTA)
    if content:
        m.content_begin(a.level)
    fn()


def kernels_only(a):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    n = 128
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    d = noisy_frames(n, gen)
    L, fb = _capi.yuv420_layout("nv12", W, H)
    y = torch.randint(16, 236, (n, fb), device="cuda", generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize()
    for _ in range(3):
        observe(m, lambda: m.observe_frames_dev(d.data_ptr(), n, W, H), a, True, False)
        observe(m, lambda: m.observe_frames_dev(d.data_ptr(), n, W, H), a, False, True)
        observe(m, lambda: m.observe_frames_dev(d.data_ptr(), n, W, H), a, True, True)
        observe(m, lambda: m.observe_frames_yuv420_dev(y.data_ptr(), n, W, H, L, fb), a, True, True)
    del d, y
    big = torch.randint(0, 256, (n, 2 * H, 2 * W, 3), device="cuda", generator=gen, dtype=torch.uint8)
    torch.cuda.synchronize()
    m.set_working_size(W, H)
    for _ in range(3):
        observe(m, lambda: m.observe_frames_dev(big.data_ptr(), n, 2 * W, 2 * H), a, True, True)
    assert m.content_info() == {"aw": W, "ah": H, "frames": n, "level": a.level} and m.activity_info()["pairs"] == n - 1
    for _ in range(3):
        m.content_box(a.min_share, a.min_fill)
    m.activity_end(); m.content_end()
    m.close()


def rate(a, res):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261019)
    n = a.frames
    # one matcher per kind of session, so that a repetition begins again (which empties an accumulator and keeps its buffers) and
    # no allocation of another kind's repetition falls into the timed interval
    kinds = {"activity": (True, False), "content": (False, True), "both": (True, True)}
    ms = {k: _capi.Matcher(_capi.default_config(nfeatures=1000)) for k in kinds}
    d = noisy_frames(n, gen)
    pin = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
    pin.copy_(d)
    host = pin.numpy()
    L, fb = _capi.yuv420_layout("nv12", W, H)
    ypin = torch.empty((n, fb), dtype=torch.uint8, pin_memory=True)
    ypin.copy_(torch.randint(16, 236, (n, fb), device="cuda", generator=gen, dtype=torch.uint8))
    yhost = ypin.numpy()
    sources = {"host_bgr_pinned": lambda m: m.observe_frames(host), "host_nv12_pinned": lambda m: m.observe_frames_yuv420(yhost, W, H, L),
               "device_bgr": lambda m: m.observe_frames_dev(d.data_ptr(), n, W, H)}

    def one(m, fn, act, cnt):
        if act:
            m.activity_begin(DELTA)
        if cnt:
            m.content_begin(a.level)
        fn(m)
    runs = {}
    for src, fn in sources.items():
        for name, (act, cnt) in kinds.items():
            runs["%s_%s" % (src, name)] = (lambda fn=fn, m=ms[name], act=act, cnt=cnt: one(m, fn, act, cnt))
    r = timed(runs, a.reps)
    for k, v in r.items():
        report("rate: " + k, v, n)
    res["rate_ms"] = r
    res["both_over_two_passes"] = {s: r[s + "_both"]["median"] / (r[s + "_activity"]["median"] + r[s + "_content"]["median"]) for s in sources}
    print("rate: both sessions in one pass / two passes: %s" % res["both_over_two_passes"], flush=True)
    assert ms["both"].content_info()["frames"] == n and ms["both"].activity_info()["pairs"] == n - 1
    for m in ms.values():
        m.activity_end(); m.content_end()
        m.close()


def recording(pages, n, a, seed=20261019):
    """-> (frames [n, H, W, 3], truth [n]: the page a hold shows, -1 for a transformed frame); every frame pillarboxed"""
    rng = np.random.default_rng(seed)
    starts, i = [], 0
    while i < n:
        starts.append(i)
        i += int(rng.geometric(a.share))
    is_moved = rng.random(len(starts)) < a.moved
    base, _, _ = synth.frames(pages, int(is_moved.sum()) + 1, PW, PH, threads=NCPU)
    seq = rng.integers(0, a.level + 1, (n, H, W, 3), dtype=np.uint8)           # the bars (and, below, nothing else) stay
    truth, k = np.full(n, -1, np.int32), 0
    for j, s in enumerate(starts):
        e = starts[j + 1] if j + 1 < len(starts) else n
        if is_moved[j]:
            seq[s:e, :, X0:X0 + PW] = base[k]
            k += 1
        else:
            p = int(rng.integers(0, len(pages)))
            img = pages[p].astype(np.int16) + rng.integers(-a.noise, a.noise + 1, (PH, PW, 3))
            seq[s:e, :, X0:X0 + PW] = np.clip(img, 0, 255).astype(np.uint8)
            truth[s:e] = p
    return seq, truth


def use(a, res):
    from changed_gate_rate import stream
    n = a.frames
    pages = synth.pages(a.pages, PW, PH, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    seq, truth = recording(pages, n, a)
    d = torch.from_numpy(seq).cuda()
    torch.cuda.synchronize()
    fbb = W * H * 3

    def learn():
        m.content_begin(a.level)
        try:
            m.observe_frames_dev(d.data_ptr(), n, W, H)
            return m.content_box(a.min_share, a.min_fill)
        finally:
            m.content_end()

    box, n_content, _, _ = learn()
    want = (X0, 0, X0 + PW, PH)
    res["use"] = {"level": a.level, "min_share": a.min_share, "min_fill": a.min_fill, "t": a.t, "box": list(box), "pasted_box": list(want),
                  "n_content": n_content, "box_is_the_pasted_one": box == want}
    print("use: learnt box %s (pasted %s), %d content pixels" % (box, want, n_content), flush=True)
    lt = timed({"learn": learn}, a.reps)["learn"]
    report("use: learn (begin, observe, box, end)", lt, n)
    res["use"]["learn_ms"] = lt
    x0, y0, x1, y1 = box
    if x1 - x0 < 2 or y1 - y0 < 2:
        m.close()
        return
    region = (W, H, [(x0, y0), (x1 - 1, y0), (x1 - 1, y1 - 1), (x0, y1 - 1)], x1 - x0, y1 - y0)
    m.set_direct_similarity(a.t)

    def gated():
        m.gate_reset(None)
        out = []
        stream(m, lambda i, c: m.submit_changed_dev(d.data_ptr() + i * fbb, c, W, H), lambda t: out.append(m.collect_changed(t)), n, UNIT)
        return np.concatenate([o[0] for o in out]), np.concatenate([o[2] for o in out])

    t = {"gated_no_region": [], "gated_learnt_region": []}
    for rep in range(a.reps + 1):                                               # (rep 0 warms; the set call stays outside the timed interval)
        for k, reg in (("gated_no_region", None), ("gated_learnt_region", region)):
            if reg is None:
                m.clear_frame_region()
            else:
                m.set_frame_region(*reg)
            t0 = time.perf_counter()
            ch, v = gated()
            if rep:
                t[k].append(time.perf_counter() - t0)
            else:
                direct = ch & (v["page_idx"] >= 0) & (v["inliers"] == 0)
                res["use"][k] = {"changed_share": float(ch.mean()), "direct_share_of_changed": float(direct.sum() / max(int(ch.sum()), 1)),
                                 "direct_verdicts_name_the_shown_page": bool((v["page_idx"][direct] == truth[direct]).all()),
                                 "transformed_frames_direct": int((direct & (truth < 0)).sum())}
                print("use: %s %s" % (k, res["use"][k]), flush=True)
    res["use"]["ms"] = {k: mmm(v) for k, v in t.items()}
    for k, v in res["use"]["ms"].items():
        report("use: " + k, v, n)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--pages", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", type=int, default=32)
    ap.add_argument("--min-share", type=float, default=0.5)
    ap.add_argument("--min-fill", type=float, default=0.25)
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--moved", type=float, default=0.25)
    ap.add_argument("--noise", type=int, default=3)
    ap.add_argument("--t", type=float, default=0.9)
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
