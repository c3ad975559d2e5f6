"""Cost and use of the YUV sampling (include/slideo_amd.h "YUV sampling").  One process per mode:

  --kernels   128 1080p frames through the mask call (conversion + small images, no pages needed), three times under each of: 4:2:0
              NV12 under (bt709, limited, 8) — yuv420_to_bgr_desc_kernel<0>, the yardstick — and the seven instances of
              yuv_sampled_to_bgr_kernel: NV16 and I444 at 8 bits, 10_msb and 10_lsb, UYVY at 8 bits.  Run it under a profiler's
              kernel trace with statistics, in a run of its own: the yuv* rows are the time per 128 frames of each kernel.  It
              prints nothing but the wall times.
  --rates     host-fed match calls from PINNED memory, --frames 1080p frames against --pages pages, ORB-1000: BGR, NV12, NV16,
              UYVY and I444 of the same frames, alternated, min / median / max.
  --use       the synthetic screen recording of tools/direct_rate.py over a deck whose text is COLOURED (the synthetic deck's glyph
              rows, grey as they come, painted red, blue, green and magenta in turn; --grey-text: as they come), its full-screen
              holds encoded (numpy, float64, BT.709 limited range) to 4:4:4 (I444) and to 4:2:0 (NV12, chroma the 2x2 mean) and
              read back under the same description.  For each: the direct look-up's s_i of the holds against the page they
              show, and the share reaching --t.

    python tools/yuv_sampling_rate.py --kernels | --rates | --use [--grey-text]   [--frames 128] [--pages 100] [--reps 5] [--t 0.99]

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
from direct_rate import recording, similarity, mmm  # noqa: E402
from yuv_desc_rate import deck, dist, pinned, K709, W, H, NCPU  # noqa: E402


def encode(frames, fmt):
    """[n, H, W, 3] BGR -> [n, frame bytes] 8-bit frames of `fmt` ('nv12', 'nv16', 'uyvy', 'i444') as BT.709 limited range; chroma
    the mean of the pixels that share a sample."""
    Kr, Kb = K709
    out = []
    for f in frames:
        f = f.astype(np.float64)
        b, g, r = f[..., 0], f[..., 1], f[..., 2]
        y = Kr * r + (1.0 - Kr - Kb) * g + Kb * b
        q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
        Y = q(16.0 + y * 219.0 / 255.0)
        U, V = 128.0 + (b - y) / (2.0 * (1.0 - Kb)) * 224.0 / 255.0, 128.0 + (r - y) / (2.0 * (1.0 - Kr)) * 224.0 / 255.0
        if fmt == "i444":
            out.append(np.concatenate([Y.reshape(-1), q(U).reshape(-1), q(V).reshape(-1)]))
            continue
        h2 = lambda c: c.reshape(H, W // 2, 2).mean(axis=2)
        if fmt == "nv12":
            v2 = lambda c: c.reshape(H // 2, 2, W // 2).mean(axis=1)
            out.append(np.concatenate([Y.reshape(-1), np.stack([q(v2(h2(U))), q(v2(h2(V)))], -1).reshape(-1)]))
        elif fmt == "nv16":
            out.append(np.concatenate([Y.reshape(-1), np.stack([q(h2(U)), q(h2(V))], -1).reshape(-1)]))
        else:                                   # uyvy: U Y0 V Y1
            Yp = Y.reshape(H, W // 2, 2)
            out.append(np.stack([q(h2(U)), Yp[..., 0], q(h2(V)), Yp[..., 1]], -1).reshape(-1))
    return np.stack(out)


def colour_text(pages):
    """The deck's glyphs (dark grey levels up to 80) in saturated colours, one per band of 48 rows: the thin coloured strokes 4:2:0
    smears."""
    pal = np.array([(0, 0, 230), (230, 40, 0), (0, 150, 0), (200, 0, 200)], np.uint8)          # BGR: red, blue, green, magenta
    out = []
    for p in pages:
        p = np.array(p, np.uint8)
        dark = p.max(axis=2) <= 80
        band = pal[(np.arange(p.shape[0]) // 48) % len(pal)]
        p[dark] = np.broadcast_to(band[:, None, :], p.shape)[dark]
        out.append(p)
    return np.stack(out)


SAMPLING_OF = {"nv12": "420", "nv16": "422", "uyvy": "422_packed", "i444": "444"}


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    for fmt, depth in (("nv12", 8), ("nv16", 8), ("nv16", "10_msb"), ("nv16", "10_lsb"), ("i444", 8), ("i444", "10_msb"), ("i444", "10_lsb"), ("uyvy", 8)):
        b = 1 if depth == 8 else 2
        L, fb = _capi.yuv_layout(fmt, W, H, bytes_per_sample=b)
        buf = rng.integers(0, 256, (n, fb), dtype=np.uint8)
        if depth == "10_lsb":
            buf[:, 1::2] &= 3
        m.set_yuv_sampling("420")
        m.set_yuv_description("bt709", "limited", depth)
        m.set_yuv_sampling(SAMPLING_OF[fmt])
        for _ in range(3):
            t0 = time.perf_counter()
            m.changed_mask_yuv420(buf, W, H, L)
            print("kernels: %-6s depth %-7s mask call of %d frames %.1f ms" % (fmt, depth, n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.close()


def rates(a):
    res = {"shape": "%d pages, %d 1080p frames from pinned memory, ORB-1000" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    idx = np.arange(a.frames) % 32
    runs = {}
    fbgr = pinned(frames[idx].reshape(a.frames, -1))
    runs["bgr"] = (lambda: m.set_yuv_sampling("420"), lambda: m.match_frames(fbgr.numpy().reshape(a.frames, H, W, 3)))
    for fmt in ("nv12", "nv16", "uyvy", "i444"):
        buf = pinned(encode(frames, fmt)[idx])
        L = _capi.yuv_layout(fmt, W, H)[0]
        runs[fmt] = (lambda fmt=fmt: m.set_yuv_sampling(SAMPLING_OF[fmt]), lambda buf=buf, L=L: m.match_frames_yuv420(buf.numpy(), W, H, L))
    m.set_yuv_description("bt709", "limited", 8)
    t = {k: [] for k in runs}
    for prep, fn in runs.values():
        prep()
        fn()
    for _ in range(a.reps):
        for k, (prep, fn) in runs.items():
            prep()
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    for k, v in t.items():
        r = mmm(v)
        res[k] = dict(r, frames_per_s=a.frames / (r["median"] * 1e-3))
        print("rates: %-6s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (k, r["min"], r["median"], r["max"], a.frames,
                                                                                            res[k]["frames_per_s"]), flush=True)
    m.close()
    print(json.dumps(res))


def use(a):
    res = {"shape": "%d pages, the full-screen holds among %d 1080p frames of tools/direct_rate.py's screen recording, encoded as BT.709 limited "
                    "range and read under (bt709, limited, 8)" % (a.pages, a.frames)}
    pages = synth.pages(a.pages, 2001, 1125, threads=NCPU)
    if not a.grey_text:
        pages = colour_text(pages)
    res["text"] = "grey, as the synthetic deck comes" if a.grey_text else "coloured (red, blue, green, magenta by bands of 48 rows)"
    m = _capi.Matcher(_capi.default_config(nfeatures=1000))
    for i in range(0, a.pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    seq, truth, starts = recording(m, pages, a.frames, 0.5, 0.25, 3)
    tr = truth[starts]
    keep = starts[tr >= 0]
    tr = tr[tr >= 0]
    m.set_yuv_description("bt709", "limited", 8)
    for fmt in ("i444", "nv12"):
        yuv = encode(seq[keep], fmt)
        L = _capi.yuv_layout(fmt, W, H)[0]
        m.set_yuv_sampling(SAMPLING_OF[fmt])
        bgr = np.stack([m.yuv420_to_bgr(f, W, H, L) for f in yuv])
        err = np.abs(bgr.astype(np.int16) - seq[keep].astype(np.int16))
        smalls = np.stack([m.small_image(b) for b in bgr])
        ssd = m.page_small_ssd(smalls).astype(np.float64)
        npx = smalls.shape[1] * smalls.shape[2]
        rows = np.arange(len(keep))
        s_truth = similarity(ssd[rows, tr], npx)
        r = {"holds": int(len(keep)), "bgr_abs_error_vs_source": {"mean": float(err.mean()), "p99": float(np.percentile(err, 99)), "max": int(err.max())},
             "direct_s_i_full_screen_vs_shown_page": dist(s_truth),
             "direct_nearest_page_is_the_truth_share": float((ssd.argmin(axis=1) == tr).mean()),
             "direct_share_at_or_above_t": {"t": a.t, "share": float((s_truth >= a.t).mean())}}
        res[fmt] = r
        for k, x in r.items():
            print("use: %-5s %-46s %s" % (fmt, k, x), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--grey-text", action="store_true")
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
