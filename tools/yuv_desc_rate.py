"""Cost and use of the YUV colour description (include/slideo_amd.h "YUV colour description").  One process per mode:

  --kernels   128 1080p frames through the mask call (conversion + small images, no pages needed), three times under each of: the
              default and (bt709, limited, 8) over three 8-bit layouts (NV12 tight, I420 tight, NV12 with a luma pitch of 2 mod 4,
              where no dword luma load applies), then (bt709, limited, 10_msb: P010) and (bt709, limited, 10_lsb).  Run it under a
              profiler's kernel trace with statistics, in a run of its own: the yuv420_to_bgr* rows are the time per 128 frames of
              each launch (one kernel converts all of them; a library that still has yuv420_to_bgr_kernel, named by
              SLIDEO_LIB_PATH, runs that one under the default).  It prints nothing but the wall times.
  --rates     host-fed match calls from PINNED memory, --frames 1080p frames against --pages pages, ORB-1000: NV12 8-bit under the
              default against P010 under (bt709, limited, 10_msb), alternated, min / median / max.  --nv12-only: the first alone,
              through no call an older library lacks (SLIDEO_LIB_PATH: the parent commit's build, interleaved process by process).
  --use       the synthetic screen recording of tools/direct_rate.py encoded to NV12 as BT.709 limited range (numpy, float64, chroma
              the 2x2 mean), then read (1) under the default description — what every caller got so far — and (2) under
              (bt709, limited, 8).  For each: the direct look-up's s_i of the full-screen holds against the page they show and
              against the nearest wrong page, the share whose nearest page is the truth, and the pipeline's re-projection
              similarity and share assigned to the truth over all holds.

    python tools/yuv_desc_rate.py --kernels | --rates [--nv12-only] | --use   [--frames 256] [--pages 100] [--reps 5] [--t 0.99]

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

NCPU = min(16, os.cpu_count() or 1)
W, H = 1920, 1080
K709 = (0.2126, 0.0722)


def encode_bt709_limited(frames, bits=8):
    """[n, H, W, 3] BGR -> (Y [n, H, W], UV [n, H/2, W] interleaved U V) as 8-bit values, or 10-bit values (bits=10)."""
    Kr, Kb = K709
    Kg = 1.0 - Kr - Kb
    scale = 1 << (bits - 8)
    top = (1 << bits) - 1
    Ys, Cs = [], []
    for f in frames:
        f = f.astype(np.float64)
        b, g, r = f[..., 0], f[..., 1], f[..., 2]
        y = Kr * r + Kg * g + Kb * b
        cb, cr = (b - y) / (2.0 * (1.0 - Kb)), (r - y) / (2.0 * (1.0 - Kr))
        sub = lambda c: c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
        Y = 16.0 + y * 219.0 / 255.0
        U, V = 128.0 + sub(cb) * 224.0 / 255.0, 128.0 + sub(cr) * 224.0 / 255.0
        q = lambda c: np.clip(np.rint(c * scale), 0, top).astype(np.uint16)
        Ys.append(q(Y))
        Cs.append(np.stack([q(U), q(V)], -1).reshape(H // 2, W))
    return np.stack(Ys), np.stack(Cs)


def nv12(Y, C):
    return np.concatenate([Y.reshape(len(Y), -1), C.reshape(len(C), -1)], axis=1).astype(np.uint8)


def p010(Y, C):
    return (np.concatenate([Y.reshape(len(Y), -1), C.reshape(len(C), -1)], axis=1).astype(np.uint16) << 6)


def pinned(a):
    t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
    t.copy_(torch.from_numpy(a))
    return t


def deck(n_pages, nfeatures=1000):
    pages = synth.pages(n_pages, 2001, 1125, threads=NCPU)
    m = _capi.Matcher(_capi.default_config(nfeatures=nfeatures))
    for i in range(0, n_pages, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    return m, pages


def dist(x):
    x = np.asarray(x, np.float64)
    return {"min": float(x.min()), "p05": float(np.percentile(x, 5)), "median": float(np.median(x)), "p95": float(np.percentile(x, 95)),
            "max": float(x.max()), "n": int(len(x))} if len(x) else None


def kernels(a):
    m = _capi.Matcher(_capi.default_config())
    rng = np.random.default_rng(1)
    n = 128
    y8 = rng.integers(0, 256, (n, W * H * 3 // 2), dtype=np.uint8)
    y16 = (rng.integers(0, 1024, (n, W * H * 3 // 2), dtype=np.uint16))
    L8 = _capi.yuv420_layout("nv12", W, H)[0]
    Li = _capi.yuv420_layout("i420", W, H)[0]
    Lp, fbp = _capi.yuv420_layout("nv12", W, H, pitch=W + 2, row_align=2)       # luma pitch = 2 mod 4: no dword luma loads
    yp = rng.integers(0, 256, (n, fbp), dtype=np.uint8)
    L16 = _capi.yuv420_layout("nv12", W, H, bytes_per_sample=2)[0]
    for desc, name, buf, L in ((("bt601", "limited", 8), "nv12", y8, L8), (("bt709", "limited", 8), "nv12", y8, L8),
                               (("bt601", "limited", 8), "i420", y8, Li), (("bt709", "limited", 8), "i420", y8, Li),
                               (("bt601", "limited", 8), "nv12 pitch %d" % (W + 2), yp, Lp), (("bt709", "limited", 8), "nv12 pitch %d" % (W + 2), yp, Lp),
                               (("bt709", "limited", "10_msb"), "p010", y16 << 6, L16), (("bt709", "limited", "10_lsb"), "nv12 16-bit", y16, L16)):
        m.set_yuv_description(*desc)
        for _ in range(3):
            t0 = time.perf_counter()
            m.changed_mask_yuv420(buf, W, H, L)
            print("kernels: %-28s %-16s mask call of %d frames %.1f ms" % (desc, name, n, (time.perf_counter() - t0) * 1e3), flush=True)
    m.close()


def rates(a):
    res = {"shape": "%d pages, %d 1080p frames from pinned memory, ORB-1000" % (a.pages, a.frames), "lib": os.environ.get("SLIDEO_LIB_PATH", "product")}
    m, pages = deck(a.pages)
    frames, _, _ = synth.frames(pages, 32, W, H, threads=NCPU)           # 32 distinct frames, cycled
    Y, C = encode_bt709_limited(frames, 10)
    idx = np.arange(a.frames) % 32
    runs = {}
    f8 = pinned(nv12(Y >> 2, C >> 2)[idx])
    L8 = _capi.yuv420_layout("nv12", W, H)[0]
    runs["nv12_8bit_default"] = (lambda: None if a.nv12_only else m.set_yuv_description(), lambda: m.match_frames_yuv420(f8.numpy(), W, H, L8))
    if not a.nv12_only:
        f16 = pinned(p010(Y, C)[idx].view(np.uint8).reshape(a.frames, -1))
        L16 = _capi.yuv420_layout("nv12", W, H, bytes_per_sample=2)[0]
        runs["nv12_8bit_bt709"] = (lambda: m.set_yuv_description("bt709", "limited", 8), lambda: m.match_frames_yuv420(f8.numpy(), W, H, L8))
        runs["p010_bt709"] = (lambda: m.set_yuv_description("bt709", "limited", "10_msb"), lambda: m.match_frames_yuv420(f16.numpy(), W, H, L16))
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
        print("rates: %-20s min %.1f median %.1f max %.1f ms per %d frames = %.0f frames/s" % (k, r["min"], r["median"], r["max"], a.frames,
                                                                                               res[k]["frames_per_s"]), flush=True)
    m.close()
    print(json.dumps(res))


def use(a):
    res = {"shape": "%d pages, %d 1080p frames of tools/direct_rate.py's screen recording encoded to NV12 as BT.709 limited range" % (a.pages, a.frames)}
    m, pages = deck(a.pages)
    seq, truth, starts = recording(m, pages, a.frames, 0.5, 0.25, 3)
    first, tr = starts, truth[starts]
    Y, C = encode_bt709_limited(seq[first], 8)
    yuv = nv12(Y, C)
    L = _capi.yuv420_layout("nv12", W, H)[0]
    fs = tr >= 0
    for name, desc in (("read_as_default_bt601_limited", ("bt601", "limited", 8)), ("read_as_bt709_limited", ("bt709", "limited", 8))):
        m.set_yuv_description(*desc)
        bgr = np.stack([m.yuv420_to_bgr(f, W, H, L) for f in yuv])
        err = np.abs(bgr.astype(np.int16) - seq[first].astype(np.int16))
        smalls = np.stack([m.small_image(b) for b in bgr])
        ssd = m.page_small_ssd(smalls).astype(np.float64)
        npx = smalls.shape[1] * smalls.shape[2]
        rows = np.arange(len(first))
        s_truth = similarity(ssd[rows[fs], tr[fs]], npx)
        wrong = ssd.copy()
        wrong[rows[fs], tr[fs]] = np.inf
        s_wrong = similarity(wrong[fs].min(axis=1), npx)
        arg = ssd.argmin(axis=1)
        v = m.match_frames_yuv420(yuv, W, H, L)
        r = {"bgr_abs_error_vs_source": {"mean": float(err.mean()), "p99": float(np.percentile(err, 99)), "max": int(err.max())},
             "direct_s_i_full_screen_vs_shown_page": dist(s_truth), "direct_s_i_full_screen_vs_nearest_wrong_page": dist(s_wrong),
             "direct_nearest_page_is_the_truth_share": float((arg[fs] == tr[fs]).mean()),
             "direct_share_at_or_above_t": {"t": a.t, "share": float((s_truth >= a.t).mean())},
             "pipeline_similarity_all_holds": dist(v["similarity"][v["page_idx"] >= 0]),
             "pipeline_similarity_full_screen": dist(v["similarity"][fs & (v["page_idx"] >= 0)]),
             "pipeline_assigned_share": float((v["page_idx"] >= 0).mean()),
             "pipeline_full_screen_assigned_to_truth_share": float((v["page_idx"][fs] == tr[fs]).mean())}
        res[name] = r
        for k, x in r.items():
            print("use: %-30s %-46s %s" % (name, k, x), flush=True)
    m.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--rates", action="store_true")
    ap.add_argument("--nv12-only", action="store_true")
    ap.add_argument("--use", action="store_true")
    ap.add_argument("--frames", type=int, default=256)
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
