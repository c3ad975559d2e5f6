"""Cost and use of the YUV chroma filter (include/slideo_amd.h "YUV chroma filter").  One process per mode:

  --kernels   128 1080p frames through the mask call (conversion + small images, no pages needed), three times under each of NV12,
              P010, NV16 and UYVY, first under NEAREST — yuv420_to_bgr_desc_kernel<0>, <1> and two instances of
              yuv_sampled_to_bgr_kernel, the yardsticks — then under LEFT: four instances of yuv_chroma_to_bgr_kernel.  All under
              (bt709, limited).  Run it under a profiler's kernel trace with statistics, in a run of its own: the yuv* rows are
              the time per 128 frames of each kernel.  It prints nothing but the wall times.
  --rates     host-fed match calls from PINNED memory, --frames 1080p NV12 frames against --pages pages, ORB-1000, under NEAREST
              and under LEFT, alternated, min / median / max (the set-up of tools/yuv_sampling_rate.py --rates).
  --use       the coloured-text screen recording of tools/yuv_sampling_rate.py --use, its full-screen holds encoded (numpy, float64,
              BT.709 limited range) to NV12 twice — chroma the 2x2 mean (centre siting), and chroma a [1 2 1] / 4 horizontal tap on
              the even columns by the 2-row mean (left siting) — and to I444; each NV12 encoding read back under NEAREST and under
              its own filter.  For each: the mean absolute BGR error against the source, the direct look-up's s_i of the holds
              against the page they show, and the share reaching --t.

    python tools/yuv_chroma_rate.py --kernels | --rates | --use   [--frames 128] [--pages 100] [--reps 5] [--t 0.99]

Prints one line per measurement and a JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402,F401

from slideo_amd import _capi, synth  # noqa: E402
from direct_rate import recording, similarity, mmm  # noqa: E402
from yuv_desc_rate import deck, dist, pinned, K709, W, H, NCPU  # noqa: E402
from yuv_sampling_rate import colour_text, encode  # noqa: E402


def encode_nv12(frames, siting):
    """[n, H, W, 3] BGR -> [n, frame bytes] 8-bit NV12 as BT.709 limited range.  siting 'center': chroma the 2x2 mean; 'left': the
    chroma sample sits on the even luma column — [1 2 1] / 4 over columns 2k - 1, 2k, 2k + 1 (replicated at the edge) — and between
    the two luma rows: their mean."""
    if siting == "center":
        return encode(frames, "nv12")
    Kr, Kb = K709
    out = []
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    for f in frames:
        f = f.astype(np.float64)
        b, g, r = f[..., 0], f[..., 1], f[..., 2]
        y = Kr * r + (1.0 - Kr - Kb) * g + Kb * b
        Y = q(16.0 + y * 219.0 / 255.0)
        planes = []
        for c in (128.0 + (b - y) / (2.0 * (1.0 - Kb)) * 224.0 / 255.0, 128.0 + (r - y) / (2.0 * (1.0 - Kr)) * 224.0 / 255.0):
            p = np.pad(c, ((0, 0), (1, 1)), mode="edge")
            hz = (p[:, 0:-2:2] + 2.0 * p[:, 1:-1:2] + p[:, 2::2]) / 4.0            # at columns 0, 2, 4 ...
            planes.append(q(hz.reshape(H // 2, 2, W // 2).mean(axis=1)))
        out.append(np.concatenate([Y.reshape(-1), np.stack(planes, -1).reshape(-1)]))
    return np.stack(out)


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    for filt in ("nearest", "left"):
        for name, fmt, depth, sampling in (("nv12", "nv12", 8, "420"), ("p010", "nv12", "10_msb", "420"), ("nv16", "nv16", 8, "422"),
                                           ("uyvy", "uyvy", 8, "422_packed")):
            b = 1 if depth == 8 else 2
            L, fb = _capi.yuv_layout(fmt, W, H, bytes_per_sample=b)
            buf = rng.integers(0, 256, (n, fb), dtype=np.uint8)
            m.set_yuv_sampling("420")
            m.set_yuv_description("bt709", "limited", depth)
            m.set_yuv_sampling(sampling)
            m.set_yuv_chroma(filt)
            for _ in range(3):
                t0 = time.perf_counter()
                m.changed_mask_yuv420(buf, W, H, L)
                print("kernels: %-7s %-5s mask call of %d frames %.1f ms" % (filt, name, n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.close()


def rates(a):
    res = {"shape": "%d pages, %d 1080p NV12 frames from pinned memory, ORB-1000" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    idx = np.arange(a.frames) % 32
    buf = pinned(encode(frames, "nv12")[idx])
    L = _capi.yuv_layout("nv12", W, H)[0]
    m.set_yuv_description("bt709", "limited", 8)
    t = {"nearest": [], "left": []}
    for k in t:
        m.set_yuv_chroma(k)
        m.match_frames_yuv420(buf.numpy(), W, H, L)
    for _ in range(a.reps):
        for k in t:
            m.set_yuv_chroma(k)
            t0 = time.perf_counter()
            m.match_frames_yuv420(buf.numpy(), W, H, L)
            t[k].append(time.perf_counter() - t0)
    for k, v in t.items():
        r = mmm(v)
        res[k] = dict(r, frames_per_s=a.frames / (r["median"] * 1e-3))
        print("rates: %-8s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (k, r["min"], r["median"], r["max"], a.frames,
                                                                                              res[k]["frames_per_s"]), flush=True)
    m.close()
    print(json.dumps(res))


def use(a):
    res = {"shape": "%d pages, the full-screen holds among %d 1080p frames of tools/direct_rate.py's screen recording, coloured text, encoded as "
                    "BT.709 limited range and read under (bt709, limited, 8)" % (a.pages, a.frames)}
    pages = colour_text(synth.pages(a.pages, 2001, 1125, threads=NCPU))
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    seq, truth, starts = recording(m, pages, a.frames, 0.5, 0.25, 3)
    tr = truth[starts]
    keep = starts[tr >= 0]
    tr = tr[tr >= 0]
    src = seq[keep]
    m.set_yuv_description("bt709", "limited", 8)
    runs = [("i444", "444", "nearest", lambda: encode(src, "i444"), "i444")]
    for siting, own in (("center", "center"), ("left", "left")):
        for filt in ("nearest", own):
            runs.append(("nv12 %s-sited, read %s" % (siting, filt), "420", filt, lambda siting=siting: encode_nv12(src, siting), "nv12"))
    cache = {}
    for name, sampling, filt, enc, fmt in runs:
        key = name.split(",")[0]
        if key not in cache:
            cache = {key: enc()}
        yuv = cache[key]
        L = _capi.yuv_layout(fmt, W, H)[0]
        m.set_yuv_sampling(sampling)
        m.set_yuv_chroma(filt)
        bgr = np.stack([m.yuv420_to_bgr(f, W, H, L) for f in yuv])
        err = np.abs(bgr.astype(np.int16) - src.astype(np.int16))
        smalls = np.stack([m.small_image(b) for b in bgr])
        ssd = m.page_small_ssd(smalls).astype(np.float64)
        npx = smalls.shape[1] * smalls.shape[2]
        rows = np.arange(len(keep))
        s_truth = similarity(ssd[rows, tr], npx)
        r = {"holds": int(len(keep)), "bgr_abs_error_vs_source": {"mean": float(err.mean()), "p99": float(np.percentile(err, 99)), "max": int(err.max())},
             "direct_s_i_full_screen_vs_shown_page": dist(s_truth),
             "direct_nearest_page_is_the_truth_share": float((ssd.argmin(axis=1) == tr).mean()),
             "direct_share_at_or_above_t": {"t": a.t, "share": float((s_truth >= a.t).mean())}}
        res[name] = r
        for k, x in r.items():
            print("use: %-34s %-46s %s" % (name, k, x), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--pages", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--t", type=float, default=0.99)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    if a.rates:
        rates(a)
    if a.use:
        use(a)


if __name__ == "__main__":
    main()
